// hair_batch.hip — the four yocto::extension functions as unit-level batches (gfx950): yh_hair_brdf_batch, _eval_, _pdf_, _sample_.
// Outside csrc/, as every unit-level kernel: an edit here leaves the sample-loop kernels' translation units alone.
// Compiled with -ffp-contract=off (see dev_math.h).
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "hair_params.h"

using namespace yhd;

// hair_brdf as 30 floats (yhair.h): sigma_a[3] alpha eta h v[4] s sin[3]
// cos[3] gamma_o world_to_brdf[12]
YH_DEV void unpack_brdf(const float* b, yhd_material& m, hair_hit& hh) {
  m.sigma_a[0] = b[0], m.sigma_a[1] = b[1], m.sigma_a[2] = b[2];
  m.alpha = b[3], m.eta = b[4];
  hh.h = b[5];
  for (int p = 0; p < 4; p++) m.v[p] = b[6 + p];
  m.s = b[10];
  for (int k = 0; k < 3; k++) m.sin_2k_alpha[k] = b[11 + k], m.cos_2k_alpha[k] = b[14 + k];
  hh.gamma_o = b[17];
  hh.w2b     = ldframe(b + 18);
  derive_material(m);
}

// eval_hair_brdf (ext.cpp:127-177) entirely on the device; mats: the public struct itself (include/yhair.h)
__global__ void k_hair_brdf(int n, const yh_material* mats, const float* v, const float* nrm,
    const float* tng, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const yh_material& m = mats[i];
  f3 sigma_a = mk3(0.0f);
  f3 msa = ld3(m.sigma_a), col = ld3(m.color);
  if (!is_zero(msa)) {
    sigma_a = msa;
  } else if (!is_zero(col)) {  // sigma_a_from_reflectance (ext.cpp:121-125)
    float bn  = m.beta_n;
    float den = 5.969f - 0.215f * bn + 2.532f * sqr(bn) - 10.73f * powt<3>(bn) +
                5.574f * powt<4>(bn) + 0.245f * powt<5>(bn);
    f3 q    = f3{logf(col.x), logf(col.y), logf(col.z)} / den;
    sigma_a = q * q;
  } else if (m.eumelanin != 0 || m.pheomelanin != 0) {  // ext.cpp:115-119
    sigma_a = m.eumelanin * f3{0.419f, 0.697f, 1.37f} + m.pheomelanin * f3{0.187f, 0.4f, 1.05f};
  }
  float* o = out + 30 * (size_t)i;
  o[0] = sigma_a.x, o[1] = sigma_a.y, o[2] = sigma_a.z;
  o[3] = m.alpha, o[4] = m.eta;
  hair_hit hh = hair_setup(v[i], ld3(nrm + 3 * i), ld3(tng + 3 * i));
  o[5]     = hh.h;
  yhd_material t;
  hair_roughness_terms(m.beta_m, m.beta_n, m.alpha, t);
  for (int p = 0; p < 4; p++) o[6 + p] = t.v[p];
  o[10] = t.s;
  for (int k = 0; k < 3; k++) o[11 + k] = t.sin_2k_alpha[k], o[14 + k] = t.cos_2k_alpha[k];
  o[17] = hh.gamma_o;
  const frame& w = hh.w2b;
  o[18] = w.x.x, o[19] = w.x.y, o[20] = w.x.z, o[21] = w.y.x, o[22] = w.y.y, o[23] = w.y.z;
  o[24] = w.z.x, o[25] = w.z.y, o[26] = w.z.z, o[27] = w.o.x, o[28] = w.o.y, o[29] = w.o.z;
}
// eval and pdf run the INTEGRATOR's code path: one quad (four threads) per item,
// lobe p on lane p (hair_eval_pdf_quad). The scalar hair_eval_pdf<> is what the
// self-test kernel uses, so both formulations are checked against the reference.
// One body: PDF false writes the value (3 floats per item), true the pdf (1 float).
template <bool PDF>
__global__ void k_hair_eval_pdf(int n, const float* brdf, const float* wo, const float* wi, float* out) {
  int  i     = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  bool valid = i < n;
  if (!valid) i = n - 1;  // keep whole quads converged
  yhd_material m;
  hair_hit     hh;
  unpack_brdf(brdf + 30 * (size_t)i, m, hh);
  f3    f;
  float pdf;
  hair_eval_pdf_quad(m, hh, ld3(wo + 3 * i), ld3(wi + 3 * i), f, pdf);
  if (!valid || (threadIdx.x & 3) != 0) return;
  if (PDF) out[i] = pdf;
  else out[3 * i] = f.x, out[3 * i + 1] = f.y, out[3 * i + 2] = f.z;
}
__global__ void k_hair_sample(int n, const float* brdf, const float* wo, const float* rn, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  yhd_material m;
  hair_hit     hh;
  unpack_brdf(brdf + 30 * (size_t)i, m, hh);
  f3 w = hair_sample(m, hh, ld3(wo + 3 * i), rn[2 * i], rn[2 * i + 1]);
  out[3 * i] = w.x, out[3 * i + 1] = w.y, out[3 * i + 2] = w.z;
}

extern "C" {
int yhk_hair_brdf(int n, const void* mats, const float* v, const float* nrm, const float* tng, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_hair_brdf, dim3((n + 255) / 256), dim3(256), 0, s, n, (const yh_material*)mats, v, nrm, tng, out);
  return (int)hipGetLastError();
}
int yhk_hair_eval(int n, const float* brdf, const float* wo, const float* wi, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_hair_eval_pdf<false>, dim3((n + 63) / 64), dim3(256), 0, s, n, brdf, wo, wi, out);
  return (int)hipGetLastError();
}
int yhk_hair_pdf(int n, const float* brdf, const float* wo, const float* wi, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_hair_eval_pdf<true>, dim3((n + 63) / 64), dim3(256), 0, s, n, brdf, wo, wi, out);
  return (int)hipGetLastError();
}
int yhk_hair_sample(int n, const float* brdf, const float* wo, const float* rn, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_hair_sample, dim3((n + 255) / 256), dim3(256), 0, s, n, brdf, wo, rn, out);
  return (int)hipGetLastError();
}
}
