// wide.hip — the sample-loop kernels that give a path MORE than four lanes (gfx950): octets over 8-wide nodes (YH_SHAPE_OCT,
// _OCT_PAIRS), sixteen lanes over 16-wide nodes (_HEX, _HEX_GROUPS) and the side-by-side launch (_SBS: quads + the top items as octets in one kernel).
// A translation unit beside csrc/kernels.hip's quad forms (together they took 77 s to compile); same templates (csrc/dev_items.h), same bits.
// Compiled with -ffp-contract=off (see dev_math.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "yhair.h"
#include "launchers.h"
#include "dev_items.h"

extern "C" {

// the kernel of a wide launch shape, or NULL when this build does not contain it. Of the instrumented builds, only those the table of launch
// shapes lists (csrc/yh_device.h: yhd_shapes; the 8-wide forms on plain scenes: their per-quad counters count an octet twice, the wave-level ones hold).
trace_kernel_t yhk_wide_kernel(int counted, int general, int shape) {
  if (counted && !(general ? yhd_shapes[shape].counted_general : yhd_shapes[shape].counted_plain)) return nullptr;
  if (shape == YH_SHAPE_OCT && counted && !general) return k_trace<true, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_OCT>;
  if (shape == YH_SHAPE_OCT && !counted) return general ? k_trace<false, true, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_OCT> : k_trace<false, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_OCT>;
  if (shape == YH_SHAPE_HEX && !counted) return general ? k_trace<false, true, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_HEX> : k_trace<false, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_HEX>;
  if (shape == YH_SHAPE_HEX && counted && !general) return k_trace<true, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_HEX>;
  if (shape == YH_SHAPE_OCT_PAIRS && !counted) return general ? k_trace<false, true, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_OCTP> : k_trace<false, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_OCTP>;
  if (shape == YH_SHAPE_HEX_GROUPS && !counted) return general ? k_trace<false, true, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_HEXP> : k_trace<false, false, YH_OCT_BLOCK, YH_MIN_WAVES, YH_MODE_HEXP>;
  return nullptr;
}

// (side by side: both forms at YH_BLOCK threads; the LDS of the larger layout)
static size_t sbs_lds(const yhd_scene* sc) {
  // (per form: its stacks in front of the tables and, behind them, its records of the ONCE form)
  const size_t quads  = (size_t)(sc->stack_entries + YH_HITROWS) * (YH_BLOCK / 4) * 4 + (size_t)YHD_ONCE_F4(sc, YH_BLOCK / 4) * 16;
  const size_t octets = (size_t)(sc->stack_entries8 + YH_HITROWS) * (YH_BLOCK / 8) * 4 + (size_t)YHD_ONCE_F4(sc, YH_BLOCK / 8) * 16;
  return std::max(quads, octets) + (size_t)YHD_LDS_TABLES_F4(sc) * 16;
}
int yhk_trace_sbs_lds_bytes(const yhd_scene* sc) { return (int)sbs_lds(sc); }
// (asked of the variant without the ONCE form, as yhk_trace_occupancy)
int yhk_trace_sbs_occupancy(int lds_bytes, int general) {
  int  blocks = 0;
  auto k      = general ? k_trace_sbs<true> : k_trace_sbs<false>;
  if (lds_bytes > 64 * 1024 && hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, YH_BLOCK, lds_bytes) != hipSuccess) return 1;
  return blocks < 1 ? 0 : blocks;
}
int yhk_trace_sbs(const yhd_scene* sc, const yhd_state* st, int nsamples, int oct_blocks, int quad_items, int oct_entries, int grid_blocks,
    hipStream_t stream) {
  const size_t lds = sbs_lds(sc);
  const bool   once = sc->scene_once > 0;
  auto         k    = sc->general_materials ? k_trace_sbs<true> : sc->lights_const_env ? (once ? k_trace_sbs_cenv<true> : k_trace_sbs_cenv<false>) : once ? k_trace_sbs<false, true> : k_trace_sbs<false>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3(grid_blocks), dim3(YH_BLOCK), lds, stream, *sc, *st, nsamples, oct_blocks, quad_items, oct_entries);
  return (int)hipGetLastError();
}
}
