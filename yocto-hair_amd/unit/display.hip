// display.hip — yh_download_display: the last step of the interactive caller's reset_display, tonemap(render, exposure) followed by
// float_to_byte (apps/ysceneitraces/ysceneitraces.cpp:280,296; yocto_math.h:3820-3829, 3721-3729), on the device, so that a front end
// reads back four bytes per pixel and not sixteen; and the same of a float4 image (yh_denoise_display). A translation unit of its own: the sample-loop units do not see it.
// Not a hot path: the library's exp2f / powf, IEEE divisions (-ffp-contract=off like every unit), one lane per pixel.
#include <hip/hip_runtime.h>

#include "../csrc/yh_device.h"
#include "../csrc/launchers.h"

namespace {

// rgb_to_srgb (yocto_math.h:3746-3749)
__device__ float rgb_to_srgb(float rgb) { return (rgb <= 0.0031308f) ? 12.92f * rgb : (1 + 0.055f) * powf(rgb, 1 / 2.4f) - 0.055f; }
// tonemap_filmic, the fitted ACES curve (yocto_math.h:3788-3794)
__device__ float tonemap_filmic(float hdr_) {
  float hdr = hdr_ * 0.6f;
  float ldr = (hdr * hdr * 2.51f + hdr * 0.03f) / (hdr * hdr * 2.43f + hdr * 0.59f + 0.14f);
  return fmaxf(0.0f, ldr);
}
// float_to_byte (yocto_math.h:3729): clamp(int(a * 256), 0, 255), the clamp taken before the conversion (int() of a value beyond
// its range is undefined); a non-finite value gives 0
__device__ unsigned int float_to_byte(float a) {
  float v = a * 256;
  if (!isfinite(v) || v <= 0) return 0u;
  return v >= 255 ? 255u : (unsigned int)(int)v;
}

// one pixel: tonemap (yocto_math.h:3820-3826) of c, then the bytes, alpha among them
__device__ unsigned int display_pixel(float c[3], float alpha, float exposure, int filmic, int srgb) {
  for (int k = 0; k < 3; k++) {
    float rgb = c[k];
    if (exposure != 0) rgb *= exp2f(exposure);
    if (filmic) rgb = tonemap_filmic(rgb);
    if (srgb) rgb = rgb_to_srgb(rgb);
    c[k] = rgb;
  }
  return float_to_byte(c[0]) | float_to_byte(c[1]) << 8 | float_to_byte(c[2]) << 16 | float_to_byte(alpha) << 24;
}

__global__ void k_display(const yhd_state st, int samples, float exposure, int filmic, int srgb, unsigned int* rgba8) {
  const size_t npix = (size_t)st.width * st.height;
  const size_t pix  = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const int i = (int)(pix % st.width), j = (int)(pix / st.width);
  const int tile = (j / YH_TILE) * st.tiles_x + i / YH_TILE;
  unsigned int out = 0;  // pixels of other shards, and an image without samples (k_resolve: zeros)
  if (tile % st.shard_world == st.shard_rank && samples > 0) {
    const yhd_float4 a = st.accum[pix];
    const float      n = (float)samples;
    float c[3] = {a.x / n, a.y / n, a.z / n};
    out = display_pixel(c, a.w / n, exposure, filmic, srgb);
  }
  rgba8[pix] = out;
}

// the same of a float4 image (yh_denoise_display)
__global__ void k_display_image(const yhd_float4* image, size_t npix, float exposure, int filmic, int srgb, unsigned int* rgba8) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const yhd_float4 a = image[pix];
  float c[3] = {a.x, a.y, a.z};
  rgba8[pix] = display_pixel(c, a.w, exposure, filmic, srgb);
}

}  // namespace

// rgba8: width x height dwords in device memory; `samples` = samples accumulated per pixel
extern "C" int yhk_display(const yhd_state* st, int samples, float exposure, int filmic, int srgb, void* rgba8, hipStream_t stream) {
  const size_t npix = (size_t)st->width * st->height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_display, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, *st, samples, exposure, filmic, srgb, (unsigned int*)rgba8);
  return (int)hipGetLastError();
}
// ... of a float4 image, width x height pixels in device memory
extern "C" int yhk_display_image(const void* rgba, int width, int height, float exposure, int filmic, int srgb, void* rgba8, hipStream_t stream) {
  const size_t npix = (size_t)width * height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_display_image, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const yhd_float4*)rgba, npix, exposure, filmic, srgb, (unsigned int*)rgba8);
  return (int)hipGetLastError();
}
