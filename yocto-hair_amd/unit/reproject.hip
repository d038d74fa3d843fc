// reproject.hip — the temporal stage over the resolved render (gfx950): yh_temporal_accumulate and friends (include/yhair.h: TEMPORAL).
// The arithmetic is unit/reproject_math.h, the text the host's yh_reproject compiles too; this file only decides which lane takes which
// pixel and where a tap comes from. A translation unit of its own, outside csrc/, so that the sample-loop units compile to the code
// they compiled to without it.
//
//   k_reproject   one lane per pixel, 256-thread blocks. Pixels are dealt in 8 x 8-tile order as k_gbuffer deals them — entry k = pixel
//                 (k & 7, k >> 3 & 7) of tile k >> 6 — so a wave is one tile, and the four bilinear taps of its lanes fall into at
//                 most a 9 x 9 window of the history: neighbouring lanes share the 64-byte halves of its lines.
//                 The history is two float4 planes, hc = {rgb, length bits} and hg = {position, id bits}: a tap is two 128-bit loads, the
//                 commit two 128-bit stores. It is read from one pair of planes and written to another, which the host swaps: a tap may
//                 read a pixel another lane commits. have_history 0 seeds the history from a first frame: no history plane is read.
//                 No value passes between lanes; no LDS.
//   k_tp_lengths  the length plane of a history as ints (yh_temporal_lengths).
// k_reproject: 44 VGPRs, no scratch, no spill, eight waves per SIMD; 0.018 ms at 720 x 720 after a camera turn, a seventh of the five a-trous
// levels it feeds (profiles/temporal/latency.txt): the launch, not the 60 - 110 MB it moves, is what it costs.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "reproject_math.h"

using namespace yht;

#define YH_TP_TILE 8

namespace {

struct GlobalHistory {
  const V4 *hc, *hg;
  int       width;
  __device__ void operator()(int x, int y, V4& c, V4& g) const {
    const size_t q = (size_t)y * width + x;
    c = hc[q], g = hg[q];
  }
};

__global__ __launch_bounds__(256) void k_reproject(const V4* rgba_in, const V4* accum, int samples, const int* object, const float* position,
    int width, int height, int tiles_x, size_t entries, const V4* hc_in, const V4* hg_in, int have_history, const Camera cam,
    const Camera pcam, int same_camera, const Motion m, const yh_temporal_params P, V4* hc_out, V4* hg_out, V4* rgba_out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= entries) return;
  const size_t tile = k >> 6;
  const int    i = (int)(tile % (size_t)tiles_x) * YH_TP_TILE + (int)(k & 7), j = (int)(tile / (size_t)tiles_x) * YH_TP_TILE + (int)((k >> 3) & 7);
  if (i >= width || j >= height) return;  // (an edge tile's entries outside the image)
  const size_t pix = (size_t)j * width + i;
  V4 c;
  if (rgba_in) {
    c = rgba_in[pix];
  } else {  // k_resolve's division (unit/framebuffer.hip)
    const V4    a = accum[pix];
    const float n = (float)samples;
    c = V4{a.x / n, a.y / n, a.z / n, a.w / n};
  }
  const int           id = object[pix];
  const F3            x  = {position[3 * pix], position[3 * pix + 1], position[3 * pix + 2]};
  const GlobalHistory f{hc_in, hg_in, width};
  const Result        r = reproject_pixel(f, i, j, width, height, c, id, x, samples, cam.f, pcam.f, same_camera != 0, m, P, have_history != 0);
  hc_out[pix] = V4{r.out.x, r.out.y, r.out.z, float_of(r.length)};
  hg_out[pix] = V4{x.x, x.y, x.z, float_of(id)};
  if (rgba_out) rgba_out[pix] = r.out;
}

__global__ __launch_bounds__(256) void k_tp_lengths(const V4* hc, size_t npix, int* lengths) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix < npix) lengths[pix] = bits_of(hc[pix].w);
}

}  // namespace

extern "C" {
// All pointers DEVICE pointers, float4 images 16-byte aligned. rgba_in NULL: accum / samples (samples >= 1). object / position: the
// centre-mode planes. have_history 0: hc_in / hg_in are not read. cam / pcam: 17 floats each, on the HOST. motion: unit/reproject_math.h's
// Motion with device pointers, on the HOST (NULL: none). hc_out / hg_out must not be hc_in / hg_in. rgba_out may be NULL, or rgba_in.
int yhk_reproject(const void* rgba_in, const void* accum, int samples, const int* object, const float* position, int width, int height,
    const void* hc_in, const void* hg_in, int have_history, const float* cam, const float* pcam, const void* motion,
    const yh_temporal_params* P, void* hc_out, void* hg_out, void* rgba_out, hipStream_t stream) {
  if (width < 1 || height < 1) return 0;
  const int    tiles_x = (width + YH_TP_TILE - 1) / YH_TP_TILE, tiles_y = (height + YH_TP_TILE - 1) / YH_TP_TILE;
  const size_t entries = (size_t)tiles_x * tiles_y * 64;
  Camera       c, pc;
  for (int k = 0; k < 17; k++) c.f[k] = cam[k], pc.f[k] = pcam[k];
  const Motion m = motion ? *(const Motion*)motion : Motion{nullptr, nullptr, nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(k_reproject, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, (const V4*)rgba_in, (const V4*)accum, samples,
      object, position, width, height, tiles_x, entries, (const V4*)hc_in, (const V4*)hg_in, have_history, c, pc, (int)same_bits(cam, pcam, 17), m,
      *P, (V4*)hc_out, (V4*)hg_out, (V4*)rgba_out);
  return (int)hipGetLastError();
}

int yhk_tp_lengths(const void* hc, int width, int height, int* lengths, hipStream_t stream) {
  const size_t npix = (size_t)width * height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_tp_lengths, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const V4*)hc, npix, lengths);
  return (int)hipGetLastError();
}
}
