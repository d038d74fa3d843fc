// selftest.hip — the four Monte-Carlo self-tests (ext.cpp:555-693) on the device (gfx950): yh_selftest. Made data-parallel with PCG32
// jump-ahead: draw counts per iteration are fixed, so sample i's stream offset is known. Outside csrc/, as every unit-level kernel.
// Compiled with -ffp-contract=off (see dev_math.h).
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_trace.h"
#include "hair_params.h"

using namespace yhd;

// PCG32 jump-ahead: state after `delta` steps of the LCG (Brown, "Random
// number generation with arbitrary strides").
YH_DEV uint64_t pcg_advance(uint64_t state, uint64_t inc, uint64_t delta) {
  uint64_t cur_mult = 6364136223846793005ULL, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta /= 2;
  }
  return acc_mult * state + acc_plus;
}
YH_DEV f3 sample_sphere(float rx, float ry) {  // math.h:4847-4852
  float z   = 2 * ry - 1;
  float r   = sqrtf(fclamp(1 - z * z, 0.0f, 1.0f));
  float phi = 2 * pif * rx;
  return f3{r * cosf(phi), r * sinf(phi), z};
}
struct selftest_args {
  int      which;
  float    beta_m, beta_n;
  uint64_t state, inc;   // rng state at the start of this (beta_m, beta_n) block's sample loop
  int      count;
  float    wo[3];        // tests 0, 1, 3
};
// out (double): [0..2] first sum, [3..5] second sum, [6] max |lum(f)/pdf - 1| as float bits via atomicMax
__global__ void k_selftest(selftest_args a, double* sums, unsigned int* worst_bits) {
  int   i = blockIdx.x * blockDim.x + threadIdx.x;
  float s0[3] = {0, 0, 0}, s1[3] = {0, 0, 0};
  float dev = 0.0f;
  if (i < a.count) {
    int   per_iter = a.which == 2 ? 5 : 3;
    rng_t rng;
    rng.inc   = a.inc;
    rng.state = pcg_advance(a.state, a.inc, (uint64_t)per_iter * (uint64_t)i);
    float h   = rand1f(rng);
    if (a.which == 0 && h == 0) h += 1.1920929e-07f;  // flt_eps
    // eval_hair_brdf(mat{beta_m, beta_n, alpha 0}, h, {0,0,1}, {1,0,0})
    yhd_material m;
    m.sigma_a[0] = m.sigma_a[1] = m.sigma_a[2] = 0;
    m.alpha = 0, m.eta = 1.55f;
    hair_roughness_terms(a.beta_m, a.beta_n, m.alpha, m);
    derive_material(m);
    hair_hit hh = hair_setup(h, f3{0, 0, 1}, f3{1, 0, 0});
    f3 wo = ld3(a.wo);
    if (a.which == 2) {
      float wx = rand1f(rng), wy = rand1f(rng);
      wo = sample_sphere(wx, wy);
    }
    float rx = rand1f(rng), ry = rand1f(rng);
    f3    f;
    float pdf;
    if (a.which == 0) {
      f3 wi = sample_sphere(rx, ry);
      hair_eval_pdf<true, false>(m, hh, wo, wi, f, pdf);
      s0[0] = f.x, s0[1] = f.y, s0[2] = f.z;
    } else {
      f3 wi = hair_sample(m, hh, wo, rx, ry);
      hair_eval_pdf<true, true>(m, hh, wo, wi, f, pdf);
      if (a.which == 1) {
        if (pdf > 0) s0[0] = f.x / pdf, s0[1] = f.y / pdf, s0[2] = f.z / pdf;
      } else if (a.which == 2) {
        if (pdf > 0) dev = fabs_(luminance(f) / pdf - 1);
      } else {
        float li = wi.z * wi.z;  // Li(w) = w.z^2 (ext.cpp:662)
        if (pdf > 0) s0[0] = f.x * li / pdf, s0[1] = f.y * li / pdf, s0[2] = f.z * li / pdf;
        f3 wu = sample_sphere(rx, ry);
        f3 fu;
        hair_eval_pdf<true, false>(m, hh, wo, wu, fu, pdf);
        float lu = wu.z * wu.z;
        s1[0] = fu.x * lu, s1[1] = fu.y * lu, s1[2] = fu.z * lu;
      }
    }
  }
  // wave reduction, then one atomic per wave (sums are tiny: double atomics)
  for (int k = 0; k < 3; k++) {
    double a0 = s0[k], a1 = s1[k];
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_down(a0, off, 64);
      a1 += __shfl_down(a1, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&sums[k], a0);
      atomicAdd(&sums[3 + k], a1);
    }
  }
  for (int off = 32; off > 0; off >>= 1) dev = fmaxf(dev, __shfl_down(dev, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(worst_bits, __float_as_uint(dev));
}

extern "C" int yhk_selftest(int which, float beta_m, float beta_n, uint64_t state, uint64_t inc, int count, const float* wo,
    double* sums, unsigned int* worst_bits, hipStream_t s) {
  selftest_args a;
  a.which = which, a.beta_m = beta_m, a.beta_n = beta_n, a.state = state, a.inc = inc, a.count = count;
  a.wo[0] = wo[0], a.wo[1] = wo[1], a.wo[2] = wo[2];
  hipLaunchKernelGGL(k_selftest, dim3((count + 255) / 256), dim3(256), 0, s, a, sums, worst_bits);
  return (int)hipGetLastError();
}
