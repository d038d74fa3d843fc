// surface_batch.hip — the surface lobes and the lobe dispatch of non-hair materials as unit-level batches (gfx950): yh_surface_lobe_batch,
// yh_surface_bsdf_batch. Outside csrc/, as every unit-level kernel: an edit here leaves the sample-loop kernels' translation units alone.
// Compiled with -ffp-contract=off (see dev_math.h).
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_surface.h"

using namespace yhd;

// One surface lobe per launch (include/yhair.h YH_LOBE_*): the unit-level
// counterpart of yocto_math.h:4427-4755 for the parity tests.
__global__ void k_surface_lobe(int kind, int n, const float* params, const float* normal, const float* wo_,
    const float* wi_, const float* rn, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* q = params + 8 * (size_t)i;
  float ior = q[0], rough = q[1];
  f3    eta = ld3(q + 2), etak = ld3(q + 5);
  f3    nn = ld3(normal + 3 * (size_t)i), wo = ld3(wo_ + 3 * (size_t)i), wi = ld3(wi_ + 3 * (size_t)i);
  float rnl = rn[3 * (size_t)i], rx = rn[3 * (size_t)i + 1], ry = rn[3 * (size_t)i + 2];
  f3    f = mk3(0.0f), w = mk3(0.0f);
  float pdf = 0;
  switch (kind) {
    case 0:
      f = eval_diffuse_reflection(nn, wo, wi), pdf = sample_diffuse_reflection_pdf(nn, wo, wi);
      w = sample_diffuse_reflection(nn, wo, rx, ry);
      break;
    case 1:
      f = eval_microfacet_reflection(ior, rough, nn, wo, wi), pdf = sample_microfacet_reflection_pdf(rough, nn, wo, wi);
      w = sample_microfacet_reflection(rough, nn, wo, rx, ry);
      break;
    case 2:
      f   = eval_microfacet_reflection(eta, etak, rough, nn, wo, wi);
      pdf = sample_microfacet_reflection_pdf(rough, nn, wo, wi);
      w   = sample_microfacet_reflection(rough, nn, wo, rx, ry);
      break;
    case 3:
      f = eval_microfacet_transmission(rough, nn, wo, wi), pdf = sample_microfacet_transmission_pdf(rough, nn, wo, wi);
      w = sample_microfacet_transmission(rough, nn, wo, rx, ry);
      break;
    case 4:
      f   = eval_microfacet_refraction(ior, rough, nn, wo, wi);
      pdf = sample_microfacet_refraction_pdf(ior, rough, nn, wo, wi);
      w   = sample_microfacet_refraction(ior, rough, nn, wo, rnl, rx, ry);
      break;
    case 5:
      f = eval_delta_reflection(ior, nn, wo, wi), pdf = sample_delta_reflection_pdf(nn, wo, wi);
      w = sample_delta_reflection(nn, wo);
      break;
    case 6:
      f = eval_delta_reflection(eta, etak, nn, wo, wi), pdf = sample_delta_reflection_pdf(nn, wo, wi);
      w = sample_delta_reflection(nn, wo);
      break;
    case 7:
      f = eval_delta_transmission(nn, wo, wi), pdf = sample_delta_transmission_pdf(nn, wo, wi);
      w = sample_delta_transmission(nn, wo);
      break;
    case 8:
      f = eval_delta_refraction(ior, nn, wo, wi), pdf = sample_delta_refraction_pdf(ior, nn, wo, wi);
      w = sample_delta_refraction(ior, nn, wo, rnl);
      break;
    default: break;
  }
  float* o = out + 7 * (size_t)i;
  o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = pdf, o[4] = w.x, o[5] = w.y, o[6] = w.z;
}
// eval_brdf + lobe dispatch (pt.cpp:405-471, 1069-1280) of non-hair materials;
// 29 floats per item (YH_SURFACE_BSDF_FLOATS in include/yhair.h)
__global__ void k_surface_bsdf(int n, const yhd_material* mats, const float* normal, const float* wo_,
    const float* wi_, const float* rn, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f3    nn = ld3(normal + 3 * (size_t)i), wo = ld3(wo_ + 3 * (size_t)i), wi = ld3(wi_ + 3 * (size_t)i);
  float rnl = rn[3 * (size_t)i], rx = rn[3 * (size_t)i + 1], ry = rn[3 * (size_t)i + 2];
  surface_brdf_t b = surface_brdf(mats[i], nn, wo);
  float* o = out + 29 * (size_t)i;
  f3 lobes[5] = {b.diffuse, b.specular, b.metal, b.transmission, b.refraction};
  for (int k = 0; k < 5; k++) o[3 * k] = lobes[k].x, o[3 * k + 1] = lobes[k].y, o[3 * k + 2] = lobes[k].z;
  o[15] = b.roughness, o[16] = b.opacity;
  o[17] = b.diffuse_pdf, o[18] = b.specular_pdf, o[19] = b.metal_pdf, o[20] = b.transmission_pdf;
  o[21] = b.refraction_pdf;
  f3    f, w;
  float pdf;
  if (!is_delta(b)) {
    surface_eval_pdf(b, nn, wo, wi, f, pdf);
    w = surface_sample(b, nn, wo, rnl, rx, ry);
  } else {
    surface_eval_pdf_delta(b, nn, wo, wi, f, pdf);
    w = surface_sample_delta(b, nn, wo, rnl);
  }
  o[22] = f.x, o[23] = f.y, o[24] = f.z, o[25] = pdf, o[26] = w.x, o[27] = w.y, o[28] = w.z;
}

extern "C" {
int yhk_surface_lobe(int kind, int n, const float* params, const float* normal, const float* wo, const float* wi,
    const float* rn, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_surface_lobe, dim3((n + 255) / 256), dim3(256), 0, s, kind, n, params, normal, wo, wi, rn, out);
  return (int)hipGetLastError();
}
int yhk_surface_bsdf(int n, const void* mats, const float* normal, const float* wo, const float* wi, const float* rn,
    float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_surface_bsdf, dim3((n + 255) / 256), dim3(256), 0, s, n, (const yhd_material*)mats, normal, wo, wi, rn, out);
  return (int)hipGetLastError();
}
}
