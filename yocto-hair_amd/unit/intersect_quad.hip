// intersect_quad.hip — closest hits with a quad (or an octet) per ray (gfx950): through the PLAIN traversal of the sample-loop kernels
// (yh_intersect_plain_batch) and through the memory-table form (yh_intersect_batch). Outside csrc/, as
// unit/lights_quad.hip: it adds no device code to the sample-loop kernels' translation units.
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_path.h"

using namespace yhd;

// four threads (one quad) per ray; block of 256 threads = 64 quads
__global__ __launch_bounds__(256) void k_intersect(const yhd_scene sc, int n, const float* rays, int* object,
    int* element, float* uv, float* dist) {
  __shared__ unsigned int stacks[(YH_QSTACK + YH_HITROWS) * 64];
  int  i     = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  bool valid = i < n;
  if (!valid) i = n - 1;  // whole quads stay converged; surplus quads redo the last ray
  trace_ctx tc;
  tc.sc = &sc, tc.stats = nullptr, tc.lds_scene = nullptr, tc.ls = nullptr, tc.sc_dev = nullptr, tc.lds_lights = nullptr, tc.lds_envtab = nullptr, tc.lds_mats = nullptr;
  tc.lds_stack   = (YH_LDS unsigned int*)stacks + (threadIdx.x >> 2);
  const float* r = rays + 8 * (size_t)i;
  ray_t ray      = ray_t{ld3(r), ld3(r + 3), r[6], r[7]};
  hit_t h        = trace_ray<false, 64>(tc, ray, -1);
  if (valid && (threadIdx.x & 3) == 0) {
    object[i] = h.object, element[i] = hit_element(sc, h);
    uv[2 * i] = h.u, uv[2 * i + 1] = h.v, dist[i] = h.distance;
  }
}

// trace_ray<false, GROUPS, true, MODE> — the scene level read from its LDS copy, no second code path for memory — as the 512-thread
// kernels run it: a quad per ray over 4-wide nodes (shape 0 and the quad half of shape 5) or an octet per ray over 8-wide nodes (the
// octet half of shape 5), tables staged as a launch stages them (dev_trace.h: stage_tables), and the form that resolves the scene
// level once per ray (ONCE) where a launch on this scene takes it (yhd_scene::scene_once). k_intersect, behind yh_intersect_batch,
// runs the memory-table form, which no plain sample-loop kernel uses.
#define YH_UQ_BLOCK 512
template <int MODE, bool ONCE>
__global__ __launch_bounds__(YH_UQ_BLOCK) void k_intersect_plain(const yhd_scene sc, int n, const float* rays, int* object, int* element,
    float* uv, float* dist) {
  constexpr int LPP = YH_IS_OCT(MODE) ? 8 : 4, GROUPS = YH_UQ_BLOCK / LPP;
  extern __shared__ v4f lds_dyn[];
  YH_LDS unsigned int* lds_stack = (YH_LDS unsigned int*)lds_dyn;
  YH_LDS v4f*          lds_tabs  = (YH_LDS v4f*)(lds_stack + ((YH_IS_OCT(MODE) ? sc.stack_entries8 : sc.stack_entries) + YH_HITROWS) * GROUPS);
  trace_ctx tc;
  tc.sc = &sc, tc.ls = nullptr, tc.sc_dev = nullptr, tc.stats = nullptr;
  YH_LDS float* lds_cam;
  stage_tables(sc, lds_tabs, threadIdx.x, blockDim.x, tc, lds_cam);
  __syncthreads();
  tc.lds_stack = lds_stack + (threadIdx.x / LPP);
  tc.lds_once  = ONCE ? lds_tabs + YHD_LDS_TABLES_F4(&sc) + (threadIdx.x / LPP) : nullptr;
  int  i     = (int)((blockIdx.x * blockDim.x + threadIdx.x) / LPP);
  bool valid = i < n;
  if (!valid) i = n - 1;  // whole groups stay converged; surplus groups redo the last ray
  const float* r   = rays + 8 * (size_t)i;
  const ray_t  ray = ray_t{ld3(r), ld3(r + 3), r[6], r[7]};
  const hit_t  h   = trace_ray<false, GROUPS, true, MODE, ONCE>(tc, ray, -1);
  if (valid && (threadIdx.x & (LPP - 1)) == 0) {
    object[i] = h.object, element[i] = hit_element(sc, h);
    uv[2 * i] = h.u, uv[2 * i + 1] = h.v, dist[i] = h.distance;
  }
}

extern "C" {
int yhk_intersect(const yhd_scene* sc, int n, const float* rays, int* object, int* element, float* uv, float* dist,
    hipStream_t s) {
  hipLaunchKernelGGL(k_intersect, dim3((n + 63) / 64), dim3(256), 0, s, *sc, n, rays, object, element, uv, dist);
  return (int)hipGetLastError();
}
// form 0: a quad per ray, 1: an octet per ray. The caller has checked that the scene is a plain one (its scene level in LDS).
int yhk_intersect_plain(const yhd_scene* sc, int form, int n, const float* rays, int* object, int* element, float* uv, float* dist, hipStream_t s) {
  const int  lpp = form ? 8 : 4, groups = YH_UQ_BLOCK / lpp;
  const bool once = sc->scene_once > 0;
  const int  lds  = ((form ? sc->stack_entries8 : sc->stack_entries) + YH_HITROWS) * groups * 4 + YHD_LDS_TABLES_F4(sc) * 16 + YHD_ONCE_F4(sc, groups) * 16;
  auto k = form ? (once ? k_intersect_plain<YH_MODE_OCT, true> : k_intersect_plain<YH_MODE_OCT, false>)
                : (once ? k_intersect_plain<YH_MODE_QUAD, true> : k_intersect_plain<YH_MODE_QUAD, false>);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)(((long long)n + groups - 1) / groups)), dim3(YH_UQ_BLOCK), (size_t)lds, s, *sc, n, rays, object, element, uv, dist);
  return (int)hipGetLastError();
}
}
