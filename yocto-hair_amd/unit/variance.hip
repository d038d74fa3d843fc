// variance.hip — the variance stage over the resolved render (gfx950): yh_temporal_accumulate_variance, yh_denoise_variance_image and
// friends (include/yhair.h: VARIANCE). The arithmetic is unit/variance_math.h, the text the host's forms compile too; this file only
// decides which lane takes which pixel and where a tap comes from. A translation unit of its own, outside csrc/, beside unit/reproject.hip
// and unit/denoise.hip, whose kernels stay and keep their code.
//
//   k_reproject_m     stage M. k_reproject's dealing: 8 x 8 tiles, one lane per pixel, a wave is a tile. One more float4 history plane,
//                     hm = {M1, M2, steps bits, vt}, read and written ping-pong like hc and hg: a tap is three 128-bit loads, the commit
//                     three 128-bit stores. No value passes between lanes; no LDS.
//   k_var_spatial     stage S, after M because it reads the neighbours' M_out. One lane per pixel, 256-thread 16 x 16 tiles. A tile with
//                     no pixel below min_steps (the common case once a view has settled) reads no neighbour: the vote is one
//                     __syncthreads_or. The 7 x 7 window comes from memory: it is read where a history is young — after a reset, at
//                     disocclusions — and the hm / hg lines of a 22 x 22 window stay in L1 / L2 across the tile's lanes.
//   k_var_steps       the steps plane of a moment history as ints (yh_temporal_steps).
//   k_vdn_pack        stage F's pack: k_dn_pack's three float4 planes with the variance in u.w — the slot that carried alpha, which no
//                     tap reads; the last level takes alpha from the caller's image instead. u is the plane a level writes anyway, so
//                     the filtered variance costs no extra store: a tap stays three 128-bit loads.
//   k_vdn_level       one launch per level, as k_dn_level: a 256-thread block is a 16 x 16 tile in both forms.
//     form 0          every tap, and the 3 x 3 variance pre-filter, from memory.
//     form 1          levels 0, 1, 2: the tile and its 2s halo staged in LDS as unit/denoise.hip stages them — 20 / 24 / 32 rows x 512 B x
//                     3 planes = 30 / 36 / 48 KB, the same footprint, since the variance rides in a slot that was staged already. The
//                     pre-filter reads the same staged tile: its spacing is 1 and the halo 2s >= 2 covers it. The 32-pixel row pitch is
//                     kept for unit/denoise.hip's reason: a 128-bit LDS read is served in four groups of sixteen lanes, with 16-pixel
//                     tile rows a group is {x 0-3, 12-15 of one row} + {x 4-11 of the next}, banked over 256 B = 16 pixels, so the
//                     group's sixteen addresses fall on sixteen different 16-byte slots exactly when the pitch is a multiple of 16
//                     pixels; a tap or a pre-filter neighbour only shifts all sixteen by the same offset. From level 3 on it is form 0's
//                     code. A tile whose pixels all miss stages nothing and passes through.
// Both forms run level_pixel on the same taps in the same order: the same bits. Form 1 is the faster one at every level it stages
// (profiles/variance/latency.txt: x 0.75 - 0.90 per level in the metric's view, x 0.54 - 0.79 where every pixel is hit) and the one the context
// entries run; form 0 stays reachable through yh_atrous_variance_filter_gpu as the comparison. A level costs x 1.05 - 1.17 of k_dn_level's.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_reproject_m 49 VGPRs (k_reproject: 44), k_var_spatial 39, k_var_steps 5,
// k_vdn_pack 21, k_vdn_level 42 (k_dn_level: 40), k_vdn_level_tiled<0, 1, 2> 41 each (form 1 of k_dn_level: 38); no scratch and no spill in
// any of them. Eight waves per SIMD by registers; the staged levels are held to 5 / 4 / 3 by their 30 / 36 / 48 KB (+ 256 B for the vote).
#include <hip/hip_runtime.h>

#include "variance_launchers.h"
#include "variance_math.h"

#define YH_TP_TILE 8
#define YH_DN_TILE 16
#define YH_DN_PITCH 32 /* pixels per LDS row of form 1 (see above) */

namespace {
using yha::Tap;
using yht::Camera;
using yht::Motion;
using yhv::bits_of;
using yhv::float_of;
using yhv::V4;

struct GlobalHistoryM {
  const V4 *hc, *hg, *hm;
  int       width;
  __device__ void operator()(int x, int y, V4& c, V4& g, V4& m) const {
    const size_t q = (size_t)y * width + x;
    c = hc[q], g = hg[q];
    m = hm ? hm[q] : V4{0.0f, 0.0f, 0.0f, 0.0f};  // (no moment history: steps 0)
  }
};

__global__ __launch_bounds__(256) void k_reproject_m(const V4* rgba_in, const V4* accum, int samples, const int* object, const float* position,
    const float* albedo, int width, int height, int tiles_x, size_t entries, const V4* hc_in, const V4* hg_in, const V4* hm_in, int have_history,
    const Camera cam, const Camera pcam, int same_camera, const Motion m, const yh_temporal_params P, V4* hc_out, V4* hg_out, V4* hm_out, V4* rgba_out) {
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
  const int id = object[pix];
  const F3  x  = {position[3 * pix], position[3 * pix + 1], position[3 * pix + 2]};
  float     eff[3];
  yha::pixel_albedo(albedo, pix, id, eff);
  const GlobalHistoryM f{hc_in, hg_in, hm_in, width};
  const yhv::ResultM   r = yhv::reproject_pixel_m(f, i, j, width, height, c, eff, id, x, samples, cam.f, pcam.f, same_camera != 0, m, P, have_history != 0);
  hc_out[pix] = V4{r.out.x, r.out.y, r.out.z, float_of(r.length)};
  hg_out[pix] = V4{x.x, x.y, x.z, float_of(id)};
  hm_out[pix] = yhv::plane_of(r.m);
  if (rgba_out) rgba_out[pix] = r.out;
}

__global__ __launch_bounds__(256) void k_var_spatial(const V4* hm, const V4* hg, int width, int height, const yh_temporal_params P, int min_steps, float* variance) {
  const int    px = blockIdx.x * YH_DN_TILE + (threadIdx.x & 15), py = blockIdx.y * YH_DN_TILE + (threadIdx.x >> 4);
  const bool   inside = px < width && py < height;
  const size_t pix = (size_t)py * width + px;
  const V4     cm = hm[inside ? pix : 0];
  // a tile whose histories are all long enough (or all none) reads no neighbour
  if (!__syncthreads_or(inside && yhv::spatial_needed(bits_of(cm.z), min_steps))) {
    if (inside) variance[pix] = bits_of(cm.z) > 0 ? yhv::variance_of(cm.x, cm.y) : 0.0f;  // (what spatial_pixel returns without a window)
    return;
  }
  if (!inside) return;
  const auto f = [&](int x, int y, V4& m, V4& g) {
    const size_t q = (size_t)y * width + x;
    m = hm[q], g = hg[q];
  };
  variance[pix] = yhv::spatial_pixel(f, px, py, width, height, P, min_steps);
}

__global__ __launch_bounds__(256) void k_var_steps(const V4* hm, size_t npix, int* steps) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix < npix) steps[pix] = bits_of(hm[pix].z);
}

__global__ __launch_bounds__(256) void k_vdn_pack(const V4* rgba_in, const V4* accum, int samples, size_t npix, const float* variance, const int* object,
    const float* normal, const float* position, const float* albedo, V4* u, V4* g0, V4* g1) {
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
  const Tap t = yhv::pack_pixel(yha::V4{c.x, c.y, c.z, c.w}, variance[pix], pix, object, normal, position, albedo);
  u[pix] = V4{t.u.x, t.u.y, t.u.z, t.u.w}, g0[pix] = V4{t.g0.x, t.g0.y, t.g0.z, t.g0.w}, g1[pix] = V4{t.g1.x, t.g1.y, t.g1.z, t.g1.w};
}

// a level's result: the working image again, or after the last level the albedo back, the caller's alpha, and the variance plane
struct Last {
  int          last;
  const float* albedo;
  const V4*    alpha_src;
  float        alpha_div;
  float*       out_variance;
};
__device__ void vdn_store(yha::V4* out, size_t pix, yha::V4 v, int id, const Last& L) {
  if (!L.last) {
    out[pix] = v;
    return;
  }
  const float     alpha = L.alpha_src[pix].w / L.alpha_div;  // (read before the store: out may be alpha_src)
  const yha::V4   r     = yha::remodulate(v, pix, id, L.albedo);
  if (L.out_variance) L.out_variance[pix] = v.w;
  out[pix] = yha::V4{r.x, r.y, r.z, alpha};
}

struct GlobalFetch {
  const yha::V4 *u, *g0, *g1;
  int            width;
  __device__ Tap operator()(int x, int y) const {
    const size_t i = (size_t)y * width + x;
    return Tap{u[i], g0[i], g1[i]};
  }
};

__global__ __launch_bounds__(256) void k_vdn_level(const yha::V4* u, const yha::V4* g0, const yha::V4* g1, yha::V4* out, int width, int height, int level,
    const yh_variance_params P, const Last L) {
  const int px = blockIdx.x * YH_DN_TILE + (threadIdx.x & 15), py = blockIdx.y * YH_DN_TILE + (threadIdx.x >> 4);
  if (px >= width || py >= height) return;
  const GlobalFetch f{u, g0, g1, width};
  const size_t      pix = (size_t)py * width + px;
  vdn_store(out, pix, yhv::level_pixel(f, px, py, width, height, level, P), yha::bits_of(g0[pix].w), L);
}

// form 1, LEVEL 0 .. 2
template <int LEVEL>
__global__ __launch_bounds__(256) void k_vdn_level_tiled(const yha::V4* u, const yha::V4* g0, const yha::V4* g1, yha::V4* out, int width, int height,
    const yh_variance_params P, const Last L) {
  constexpr int S = 1 << LEVEL, HALO = 2 * S, SIDE = YH_DN_TILE + 2 * HALO;  // 20, 24, 32 rows and columns
  static_assert(SIDE <= YH_DN_PITCH, "the staged row fits the pitch");
  static_assert(HALO >= 1, "the 3 x 3 pre-filter at spacing 1 stays inside the staged halo");
  __shared__ yha::V4 lu[SIDE * YH_DN_PITCH], lg0[SIDE * YH_DN_PITCH], lg1[SIDE * YH_DN_PITCH];
  const int    px = blockIdx.x * YH_DN_TILE + (threadIdx.x & 15), py = blockIdx.y * YH_DN_TILE + (threadIdx.x >> 4);
  const bool   inside = px < width && py < height;
  const size_t pix = (size_t)py * width + px;
  // a tile of misses (sky) stages nothing: every pixel of it passes through, as level_pixel would have it
  if (!__syncthreads_or(inside && yha::bits_of(g0[inside ? pix : 0].w) != -1)) {
    if (inside) vdn_store(out, pix, u[pix], -1, L);
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
  vdn_store(out, pix, yhv::level_pixel(f, px, py, width, height, LEVEL, P), yha::bits_of(f(px, py).g0.w), L);
}

}  // namespace

extern "C" {
// (the declarations and what the arguments are: unit/variance_launchers.h)
int yhk_reproject_m(const void* rgba_in, const void* accum, int samples, const int* object, const float* position, const float* albedo, int width, int height,
    const void* hc_in, const void* hg_in, const void* hm_in, int have_history, const float* cam, const float* pcam, const void* motion,
    const yh_temporal_params* P, void* hc_out, void* hg_out, void* hm_out, void* rgba_out, hipStream_t stream) {
  if (width < 1 || height < 1) return 0;
  const int    tiles_x = (width + YH_TP_TILE - 1) / YH_TP_TILE, tiles_y = (height + YH_TP_TILE - 1) / YH_TP_TILE;
  const size_t entries = (size_t)tiles_x * tiles_y * 64;
  Camera       c, pc;
  for (int k = 0; k < 17; k++) c.f[k] = cam[k], pc.f[k] = pcam[k];
  const Motion m = motion ? *(const Motion*)motion : Motion{nullptr, nullptr, nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(k_reproject_m, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, (const V4*)rgba_in, (const V4*)accum, samples, object,
      position, albedo, width, height, tiles_x, entries, (const V4*)hc_in, (const V4*)hg_in, (const V4*)hm_in, have_history, c, pc,
      (int)yht::same_bits(cam, pcam, 17), m, *P, (V4*)hc_out, (V4*)hg_out, (V4*)hm_out, (V4*)rgba_out);
  return (int)hipGetLastError();
}

int yhk_var_spatial(int width, int height, const yh_temporal_params* T, int min_steps, const void* hm, const void* hg, float* variance, hipStream_t stream) {
  if (width < 1 || height < 1) return 0;
  const dim3 grid((unsigned)((width + YH_DN_TILE - 1) / YH_DN_TILE), (unsigned)((height + YH_DN_TILE - 1) / YH_DN_TILE)), block(256);
  hipLaunchKernelGGL(k_var_spatial, grid, block, 0, stream, (const V4*)hm, (const V4*)hg, width, height, *T, min_steps, variance);
  return (int)hipGetLastError();
}

int yhk_var_steps(const void* hm, int width, int height, int* steps, hipStream_t stream) {
  const size_t npix = (size_t)width * height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_var_steps, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const V4*)hm, npix, steps);
  return (int)hipGetLastError();
}

int yhk_vdn_pack(const void* rgba_in, const void* accum, int samples, int width, int height, const float* variance, const int* object, const float* normal,
    const float* position, const float* albedo, void* u, void* g0, void* g1, hipStream_t stream) {
  const size_t npix = (size_t)width * height;
  if (!npix) return 0;
  hipLaunchKernelGGL(k_vdn_pack, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const V4*)rgba_in, (const V4*)accum, samples, npix, variance,
      object, normal, position, albedo, (V4*)u, (V4*)g0, (V4*)g1);
  return (int)hipGetLastError();
}

int yhk_vdn_level(int form, int width, int height, int level, const yh_variance_params* P, const void* u, const void* g0, const void* g1, const float* albedo,
    int last, const void* alpha_src, float alpha_div, void* out, float* out_variance, hipStream_t stream) {
  if (width < 1 || height < 1) return 0;
  const dim3 grid((unsigned)((width + YH_DN_TILE - 1) / YH_DN_TILE), (unsigned)((height + YH_DN_TILE - 1) / YH_DN_TILE)), block(256);
  const yha::V4 *pu = (const yha::V4*)u, *p0 = (const yha::V4*)g0, *p1 = (const yha::V4*)g1;
  const Last     L{last, albedo, (const V4*)alpha_src, alpha_div, out_variance};
  if (form == 1 && level == 0) hipLaunchKernelGGL(k_vdn_level_tiled<0>, grid, block, 0, stream, pu, p0, p1, (yha::V4*)out, width, height, *P, L);
  else if (form == 1 && level == 1) hipLaunchKernelGGL(k_vdn_level_tiled<1>, grid, block, 0, stream, pu, p0, p1, (yha::V4*)out, width, height, *P, L);
  else if (form == 1 && level == 2) hipLaunchKernelGGL(k_vdn_level_tiled<2>, grid, block, 0, stream, pu, p0, p1, (yha::V4*)out, width, height, *P, L);
  else hipLaunchKernelGGL(k_vdn_level, grid, block, 0, stream, pu, p0, p1, (yha::V4*)out, width, height, level, *P, L);
  return (int)hipGetLastError();
}
}
