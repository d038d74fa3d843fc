// denoise.hip — the edge-avoiding a-trous filter over the resolved render (gfx950): yh_denoise and friends (include/yhair.h: DENOISE).
// The arithmetic is unit/atrous_math.h, the text the host's yh_atrous_filter compiles too; this file only decides where a tap comes from.
// A translation unit of its own, outside csrc/, so that the sample-loop units compile to the code they compiled to without it.
//
//   k_dn_pack     one lane per pixel: the colour (the caller's image, or accum / samples of the context's own render), demodulated, and
//                 the two float4 guide planes {normal, id bits} {position, 0}: a tap is three 128-bit loads from then on.
//   k_dn_level    one launch per level, from one working image into the other; no value passes between workgroups inside a launch.
//                 The last level multiplies the albedo back. A 256-thread block is a 16 x 16 tile of pixels in both forms.
//     form 0      every tap from memory.
//     form 1      levels 0, 1, 2 (tap spacing s = 1, 2, 4): the block first stages its tile and the 2s halo of the three planes in LDS
//                 and taps from there with 128-bit LDS reads; from level 3 on (a halo of 16 pixels and more: 48 x 48 x 48 B does not fit
//                 beside a second block) it is form 0's code.
//                 LDS row pitch: 32 pixels = 512 B for every staged level, not the 16 + 4s the halo needs. A 128-bit LDS read is served in
//                 four groups of sixteen lanes, and with 16-pixel tile rows a group is {x 0-3, 12-15 of one row} + {x 4-11 of the next}
//                 (MI355X: lanes {0-3, 12-15, 20-27} ...), banked over 256 B = 16 pixels: the group's sixteen addresses fall on sixteen
//                 different 16-byte slots exactly when the pitch is a multiple of 16 pixels. 20 and 24 would be 2-way on four and on
//                 all of the slots. So: 20 / 24 / 32 rows x 512 B x 3 planes = 30 / 36 / 48 KB.
//                 A tile whose pixels all miss stages nothing and passes through.
// Both forms run level_pixel on the same taps in the same order: the same bits. Form 1 is the faster one at every level it stages
// (profiles/denoise/latency.txt: x 0.76 - 0.94 per level in the metric's view, x 0.53 - 0.81 where every pixel is hit) and the one the context
// entries run; form 0 stays reachable through yh_atrous_filter_gpu as the comparison. pack 27 VGPRs, form 0 40, form 1 38; no scratch, no spill.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "atrous_math.h"

using namespace yha;

#define YH_DN_TILE 16
#define YH_DN_PITCH 32 /* pixels per LDS row of form 1 (see above) */

namespace {

struct GlobalFetch {
  const V4 *u, *g0, *g1;
  int       width;
  __device__ Tap operator()(int x, int y) const {
    const size_t i = (size_t)y * width + x;
    return Tap{u[i], g0[i], g1[i]};
  }
};

__global__ __launch_bounds__(256) void k_dn_pack(const V4* rgba_in, const V4* accum, int samples, size_t npix, const int* object,
    const float* normal, const float* position, const float* albedo, V4* u, V4* g0, V4* g1, int plain) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  V4 c;
  if (rgba_in) {
    c = rgba_in[pix];
  } else {  // k_resolve's division (unit/framebuffer.hip)
    const V4    a = accum[pix];
    const float n = (float)samples;
    c = samples > 0 ? V4{a.x / n, a.y / n, a.z / n, a.w / n} : V4{0, 0, 0, 0};
  }
  if (plain) {  // no level follows: the image as it is
    u[pix] = c;
    return;
  }
  const Tap t = pack_pixel(c, pix, object, normal, position, albedo);
  u[pix] = t.u, g0[pix] = t.g0, g1[pix] = t.g1;
}

__device__ void dn_store(V4* out, size_t pix, V4 v, int id, int last, const float* albedo) { out[pix] = last ? remodulate(v, pix, id, albedo) : v; }

__global__ __launch_bounds__(256) void k_dn_level(const V4* u, const V4* g0, const V4* g1, V4* out, int width, int height, int level,
    const yh_denoise_params P, int last, const float* albedo) {
  const int px = blockIdx.x * YH_DN_TILE + (threadIdx.x & 15), py = blockIdx.y * YH_DN_TILE + (threadIdx.x >> 4);
  if (px >= width || py >= height) return;
  const GlobalFetch f{u, g0, g1, width};
  const size_t      pix = (size_t)py * width + px;
  dn_store(out, pix, level_pixel(f, px, py, width, height, level, P), bits_of(g0[pix].w), last, albedo);
}

// form 1, LEVEL 0 .. 2
template <int LEVEL>
__global__ __launch_bounds__(256) void k_dn_level_tiled(const V4* u, const V4* g0, const V4* g1, V4* out, int width, int height,
    const yh_denoise_params P, int last, const float* albedo) {
  constexpr int S = 1 << LEVEL, HALO = 2 * S, SIDE = YH_DN_TILE + 2 * HALO;  // 20, 24, 32 rows and columns
  static_assert(SIDE <= YH_DN_PITCH, "the staged row fits the pitch");
  __shared__ V4 lu[SIDE * YH_DN_PITCH], lg0[SIDE * YH_DN_PITCH], lg1[SIDE * YH_DN_PITCH];
  const int    px = blockIdx.x * YH_DN_TILE + (threadIdx.x & 15), py = blockIdx.y * YH_DN_TILE + (threadIdx.x >> 4);
  const bool   inside = px < width && py < height;
  const size_t pix = (size_t)py * width + px;
  // a tile of misses (sky) stages nothing: every pixel of it passes through, as level_pixel would have it
  if (!__syncthreads_or(inside && bits_of(g0[inside ? pix : 0].w) != -1)) {
    if (inside) dn_store(out, pix, u[pix], -1, last, albedo);
    return;
  }
  const int ox = blockIdx.x * YH_DN_TILE - HALO, oy = blockIdx.y * YH_DN_TILE - HALO;
  for (int i = threadIdx.x; i < SIDE * SIDE; i += 256) {
    const int r = i / SIDE, c = i % SIDE, gx = ox + c, gy = oy + r;
    if (gx < 0 || gx >= width || gy < 0 || gy >= height) continue;  // (never tapped: level_pixel skips what lies outside the image)
    const size_t gi = (size_t)gy * width + gx;
    const int    li = r * YH_DN_PITCH + c;
    lu[li] = u[gi], lg0[li] = g0[gi], lg1[li] = g1[gi];
  }
  __syncthreads();
  if (!inside) return;
  const auto f = [&](int x, int y) {
    const int li = (y - oy) * YH_DN_PITCH + (x - ox);
    return Tap{lu[li], lg0[li], lg1[li]};
  };
  dn_store(out, pix, level_pixel(f, px, py, width, height, LEVEL, P), bits_of(f(px, py).g0.w), last, albedo);
}

}  // namespace

extern "C" {
int yhk_dn_tile(void) { return YH_DN_TILE; }
// how many levels form 1 stages in LDS (the later ones run form 0's kernel)
int yhk_dn_tiled_levels(void) { return 3; }

// All pointers DEVICE pointers, images 16-byte aligned. rgba_in NULL: accum / samples. plain: u = the colour and nothing else (no level
// follows); else normal / position / albedo may be NULL (zeros / no demodulation).
int yhk_dn_pack(const void* rgba_in, const void* accum, int samples, int width, int height, const int* object, const float* normal,
    const float* position, const float* albedo, void* u, void* g0, void* g1, int plain, hipStream_t stream) {
  const size_t npix = (size_t)width * height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_dn_pack, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const V4*)rgba_in, (const V4*)accum, samples, npix,
      object, normal, position, albedo, (V4*)u, (V4*)g0, (V4*)g1, plain);
  return (int)hipGetLastError();
}

// One level from (u, g0, g1) into out; last: the albedo (NULL: none) is multiplied back. form 0 / 1 as above.
int yhk_dn_level(int form, int width, int height, int level, const yh_denoise_params* P, const void* u, const void* g0, const void* g1,
    const float* albedo, int last, void* out, hipStream_t stream) {
  if (width < 1 || height < 1) return 0;
  const dim3 grid((unsigned)((width + YH_DN_TILE - 1) / YH_DN_TILE), (unsigned)((height + YH_DN_TILE - 1) / YH_DN_TILE)), block(256);
  const V4 *pu = (const V4*)u, *p0 = (const V4*)g0, *p1 = (const V4*)g1;
  if (form == 1 && level == 0) hipLaunchKernelGGL(k_dn_level_tiled<0>, grid, block, 0, stream, pu, p0, p1, (V4*)out, width, height, *P, last, albedo);
  else if (form == 1 && level == 1) hipLaunchKernelGGL(k_dn_level_tiled<1>, grid, block, 0, stream, pu, p0, p1, (V4*)out, width, height, *P, last, albedo);
  else if (form == 1 && level == 2) hipLaunchKernelGGL(k_dn_level_tiled<2>, grid, block, 0, stream, pu, p0, p1, (V4*)out, width, height, *P, last, albedo);
  else hipLaunchKernelGGL(k_dn_level, grid, block, 0, stream, pu, p0, p1, (V4*)out, width, height, level, *P, last, albedo);
  return (int)hipGetLastError();
}
}
