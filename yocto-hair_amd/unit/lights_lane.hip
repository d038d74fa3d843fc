// lights_lane.hip — the light code with one lane per row (gfx950): form 1 of yh_lights_batch. A translation unit of its own, outside
// csrc/, so that csrc/stream.hip compiles to the code it compiled to without it (its out-of-line device functions are allocated
// registers across all their callers in the unit).
#define YH_LANE 1
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_path.h"

using namespace yhd;

// ---------------------------------------------------------------------------------------------------------------
// yh_lights_batch, form 1: what k_stream's shading stage calls — sample_lights, lane_lights_pdf
// (out of line for the GENERAL variant) and eval_environment in their YH_LANE forms — with k_stream's tables and per-wave stack window.
// ---------------------------------------------------------------------------------------------------------------
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_lights_lanes(const yhd_scene sc, const yhd_scene* sc_dev, int n, const float* position,
    const float* direction, const float* rn, unsigned int* stack_ovf, int ovf_entries, float* out) {
  extern __shared__ v4f lds_dyn[];
  YH_LDS v4f* lds_tabs = (YH_LDS v4f*)lds_dyn;
  const int   lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  YH_LDS unsigned int* w_stack = (YH_LDS unsigned int*)(lds_tabs + YHD_LDS_TABLES_F4(&sc)) + wib * (64 * YH_LSTACK + 128);
  trace_ctx tc;
  tc.sc = &sc, tc.sc_dev = sc_dev, tc.lds_stack = nullptr, tc.stats = nullptr;
  YH_LDS float* lds_cam;
  stage_tables(sc, lds_tabs, threadIdx.x, 256, tc, lds_cam);
  __syncthreads();
  const size_t wave_id = (size_t)blockIdx.x * 4 + wib;
  lane_stack   stk;
  stk.lds = w_stack + lane, stk.ovf = stack_ovf + wave_id * (size_t)ovf_entries * 64 + lane, stk.sp = 0, stk.base = 0;
  tc.ls = &stk;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const f3     p = ld3(position + 3 * (size_t)i), d = ld3(direction + 3 * (size_t)i);
  const float* r = rn + 4 * (size_t)i;
  const f3     w     = sample_lights<false, GENERAL>(tc, p, r[0], r[1], r[2], r[3]);
  const float  pdf_w = lane_lights_pdf<GENERAL>(tc, p, w);
  const float  pdf_d = lane_lights_pdf<GENERAL>(tc, p, d);
  const f3     e     = eval_environment<false>(tc, d);
  float*       o     = out + 8 * (size_t)i;
  o[0] = w.x, o[1] = w.y, o[2] = w.z, o[3] = pdf_w, o[4] = pdf_d, o[5] = e.x, o[6] = e.y, o[7] = e.z;
}

extern "C" {
// stack_ovf: ovf_entries x 64 entries for each of the grid's (n + 255) / 256 x 4 waves
int yhk_lights_lanes(const yhd_scene* sc, const yhd_scene* sc_dev, int n, const float* position, const float* direction, const float* rn,
    unsigned int* stack_ovf, int ovf_entries, float* out, hipStream_t stream) {
  const int lds = YHD_LDS_TABLES_F4(sc) * 16 + 4 * (64 * YH_LSTACK * 4 + 64 * 8);  // tables, then a stack window per wave (as k_intersect_lanes)
  auto      k   = sc->general_materials ? k_lights_lanes<true> : k_lights_lanes<false>;  // (as yhk_stream settles its variant)
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), lds, stream, *sc, sc_dev, n, position, direction, rn, stack_ovf, ovf_entries, out);
  return (int)hipGetLastError();
}
}
