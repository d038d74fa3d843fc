// intersect_wide.hip — closest hits through the traversal of the 256-thread sample-loop kernels (gfx950): forms 2-6 of yh_intersect_plain_batch
// and their memory-table forms. Next to unit/intersect_quad.hip (forms 0 and 1, 512 threads) in a translation unit of its own, so that the
// two build side by side.
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_path.h"

using namespace yhd;

// trace_ray<false, GROUPS, LDS_SCENE, MODE> at the workgroup size — and with it the stride of the LDS stack columns — of launch shapes 1, 4, 7, 6
// and 8 (csrc/yh_device.h: yhd_shapes): a quad per ray at 64 columns (the dense form: STRIDE == 64, dot(ld, ld) per test, intersect_line's
// straight form), an octet per ray at 32 (YH_MODE_OCT, _OCTP), sixteen lanes per ray at 16 (YH_MODE_HEX, _HEXP). None of these shapes has a
// kernel with the once-per-ray scene level (csrc/kernels.hip: trace_kernel, csrc/wide.hip), so none is compiled here.
// LDS_SCENE = false: the scene level read from memory, tc.lds_scene null, as the GENERAL variants run a scene whose table does not fit LDS
// (binary scene nodes, or the 4-wide scene nodes of yhd_scene::scene_wide_root, which every quad of the octet or the sixteen runs).
#define YH_UW_BLOCK 256
template <int MODE, bool LDS_SCENE>
__global__ __launch_bounds__(YH_UW_BLOCK) void k_intersect_wide(const yhd_scene sc, int n, const float* rays, int* object, int* element,
    float* uv, float* dist) {
  constexpr int LPP = YH_IS_HEX(MODE) ? 16 : YH_IS_OCT(MODE) ? 8 : 4, GROUPS = YH_UW_BLOCK / LPP;
  extern __shared__ v4f lds_dyn[];
  YH_LDS unsigned int* lds_stack = (YH_LDS unsigned int*)lds_dyn;
  YH_LDS v4f*          lds_tabs  = (YH_LDS v4f*)(lds_stack + ((MODE == YH_MODE_QUAD ? sc.stack_entries : YH_IS_HEX(MODE) ? sc.stack_entries16 : sc.stack_entries8) + YH_HITROWS) * GROUPS);
  trace_ctx tc;
  tc.sc = &sc, tc.ls = nullptr, tc.sc_dev = nullptr, tc.stats = nullptr, tc.lds_once = nullptr;
  YH_LDS float* lds_cam;
  stage_tables(sc, lds_tabs, threadIdx.x, blockDim.x, tc, lds_cam);
  __syncthreads();
  if (!LDS_SCENE) tc.lds_scene = nullptr;
  tc.lds_stack = lds_stack + (threadIdx.x / LPP);
  int  i     = (int)((blockIdx.x * blockDim.x + threadIdx.x) / LPP);
  bool valid = i < n;
  if (!valid) i = n - 1;  // whole groups stay converged; surplus groups redo the last ray
  const float* r   = rays + 8 * (size_t)i;
  const ray_t  ray = ray_t{ld3(r), ld3(r + 3), r[6], r[7]};
  const hit_t  h   = trace_ray<false, GROUPS, LDS_SCENE, MODE>(tc, ray, -1);
  if (valid && (threadIdx.x & (LPP - 1)) == 0) {
    object[i] = h.object, element[i] = hit_element(sc, h);
    uv[2 * i] = h.u, uv[2 * i + 1] = h.v, dist[i] = h.distance;
  }
}

typedef void (*intersect_wide_t)(const yhd_scene, int, const float*, int*, int*, float*, float*);

extern "C" {
// form 2: a quad per ray (dense), 3: an octet, 4: an octet with leaf pairs, 5: sixteen lanes, 6: sixteen with leaf groups; in_memory (forms 3-6):
// the scene level read from memory. The caller has checked the form and, for the plain forms, that the scene is a plain one.
int yhk_intersect_wide(const yhd_scene* sc, int form, int in_memory, int n, const float* rays, int* object, int* element, float* uv, float* dist, hipStream_t s) {
  intersect_wide_t k = nullptr;
  switch (form) {
    case 2: k = in_memory ? nullptr : k_intersect_wide<YH_MODE_QUAD, true>; break;
    case 3: k = in_memory ? k_intersect_wide<YH_MODE_OCT, false> : k_intersect_wide<YH_MODE_OCT, true>; break;
    case 4: k = in_memory ? k_intersect_wide<YH_MODE_OCTP, false> : k_intersect_wide<YH_MODE_OCTP, true>; break;
    case 5: k = in_memory ? k_intersect_wide<YH_MODE_HEX, false> : k_intersect_wide<YH_MODE_HEX, true>; break;
    case 6: k = in_memory ? k_intersect_wide<YH_MODE_HEXP, false> : k_intersect_wide<YH_MODE_HEXP, true>; break;
    default: break;
  }
  if (!k) return (int)hipErrorInvalidValue;
  const int lpp = form >= 5 ? 16 : form >= 3 ? 8 : 4, groups = YH_UW_BLOCK / lpp;
  const int entries = lpp == 16 ? sc->stack_entries16 : lpp == 8 ? sc->stack_entries8 : sc->stack_entries;
  const int lds     = (entries + YH_HITROWS) * groups * 4 + YHD_LDS_TABLES_F4(sc) * 16;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)(((long long)n + groups - 1) / groups)), dim3(YH_UW_BLOCK), (size_t)lds, s, *sc, n, rays, object, element, uv, dist);
  return (int)hipGetLastError();
}
}
