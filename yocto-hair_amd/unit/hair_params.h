// hair_params.h — a hair material's roughness terms from its parameters (eval_hair_brdf, ext.cpp:127-147), on the device: what
// unit/hair_batch.hip's k_hair_brdf and unit/selftest.hip's k_selftest both make by hand. The integrator reads the host's table.
#ifndef YH_HAIR_PARAMS_H_
#define YH_HAIR_PARAMS_H_
#include "dev_hair.h"

namespace yhd {

template <int N>
YH_DEV float powt(float v) {  // ext.cpp:95-109
  if constexpr (N == 0) return 1;
  else if constexpr (N == 1) return v;
  else {
    float n2 = powt<N / 2>(v);
    return n2 * n2 * powt<(N & 1)>(v);
  }
}

// beta_m -> v[], beta_n -> s, alpha (degrees) -> sin / cos of 2^k alpha
YH_DEV void hair_roughness_terms(float beta_m, float beta_n, float alpha, yhd_material& m) {
  m.v[0] = sqr(0.726f * beta_m + 0.812f * sqr(beta_m) + 3.7f * powt<20>(beta_m));
  m.v[1] = 0.25f * m.v[0], m.v[2] = 4 * m.v[0], m.v[3] = m.v[2];
  m.s    = 0.626657069f * (0.265f * beta_n + 1.194f * sqr(beta_n) + 5.372f * powt<22>(beta_n));
  m.sin_2k_alpha[0] = sinf(pif / 180 * alpha);
  m.cos_2k_alpha[0] = exact_safe_sqrt(1 - sqr(m.sin_2k_alpha[0]));
  for (int k = 1; k < 3; k++) {
    m.sin_2k_alpha[k] = 2 * m.cos_2k_alpha[k - 1] * m.sin_2k_alpha[k - 1];
    m.cos_2k_alpha[k] = sqr(m.cos_2k_alpha[k - 1]) - sqr(m.sin_2k_alpha[k - 1]);
  }
}

}  // namespace yhd
#endif
