// lights_quad.hip — the light code with a quad per row (gfx950): form 0 of yh_lights_batch. The unit-level kernels of the light code live
// outside csrc/: they add no device code to the sample-loop kernels' translation units, which compile to exactly the code they compiled to
// without them.
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_path.h"

using namespace yhd;

// The light code of the sample loop on its own (yh_lights_batch, form 0): a quad per row runs sample_lights, sample_lights_pdf and
// eval_environment of dev_path.h with the tables where a launch of k_trace<GENERAL> has them (dev_trace.h: stage_tables) — the small
// lights' records, the environment cdf index and the scene level in LDS, the stack columns in front of them.
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_lights(const yhd_scene sc, int n, const float* position, const float* direction, const float* rn,
    float* out) {
  extern __shared__ v4f lds_dyn[];
  YH_LDS unsigned int* lds_stack = (YH_LDS unsigned int*)lds_dyn;
  YH_LDS v4f*          lds_tabs  = (YH_LDS v4f*)(lds_stack + (sc.stack_entries + YH_HITROWS) * 64);
  trace_ctx tc;
  tc.sc = &sc, tc.ls = nullptr, tc.sc_dev = nullptr, tc.stats = nullptr;
  YH_LDS float* lds_cam;
  stage_tables(sc, lds_tabs, threadIdx.x, blockDim.x, tc, lds_cam);
  __syncthreads();
  tc.lds_stack = lds_stack + (threadIdx.x >> 2);
  int  i     = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  bool valid = i < n;
  if (!valid) i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  const f3     p = ld3(position + 3 * (size_t)i), d = ld3(direction + 3 * (size_t)i);
  const float* r = rn + 4 * (size_t)i;
  const f3     w     = sample_lights<false, GENERAL>(tc, p, r[0], r[1], r[2], r[3]);
  const float  pdf_w = sample_lights_pdf<false, 64, GENERAL>(tc, p, w);
  const float  pdf_d = sample_lights_pdf<false, 64, GENERAL>(tc, p, d);
  const f3     e     = eval_environment<false>(tc, d);
  if (valid && (threadIdx.x & 3) == 0) {
    float* o = out + 8 * (size_t)i;
    o[0] = w.x, o[1] = w.y, o[2] = w.z, o[3] = pdf_w, o[4] = pdf_d, o[5] = e.x, o[6] = e.y, o[7] = e.z;
  }
}

extern "C" {
int yhk_lights_lds_bytes(const yhd_scene* sc) { return (sc->stack_entries + YH_HITROWS) * 64 * 4 + YHD_LDS_TABLES_F4(sc) * 16; }
int yhk_lights(const yhd_scene* sc, int n, const float* position, const float* direction, const float* rn, float* out, hipStream_t s) {
  const int lds = yhk_lights_lds_bytes(sc);
  auto      k   = sc->general_materials ? k_lights<true> : k_lights<false>;  // (as a launch settles its variant: yhk_trace)
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3((n + 63) / 64), dim3(256), lds, s, *sc, n, position, direction, rn, out);
  return (int)hipGetLastError();
}
}
