// atrous_math.h — the arithmetic of the edge-avoiding a-trous filter (Dammertz et al. 2010; include/yhair.h: DENOISE), for BOTH sides:
// the host library (g++, host/denoise.cpp: yh_atrous_filter) and the device (hipcc, unit/denoise.hip). One text; + - x / and comparisons
// only, no libm call, and neither build contracts a multiply and an add (-ffp-contract=off on the device, no FMA in the x86-64 baseline),
// so both give the same bits, as unit/object_math.h and unit/light_math.h do.
//
// A pixel is three float4: u = {working colour rgb, alpha}, g0 = {normal, the object id's bits}, g1 = {position, 0}. The working colour
// is the demodulated one, c.rgb / effective albedo; a MISS (id -1) has the effective albedo 1 whatever the albedo plane holds, so that
// it leaves the filter with the bits it came with.
#ifndef YH_ATROUS_MATH_H_
#define YH_ATROUS_MATH_H_

#include "yhair.h"

#ifdef __HIPCC__
#define YHA_HD __host__ __device__ inline
#else
#define YHA_HD inline
#endif

namespace yha {

struct V4 {
  float x, y, z, w;
};
struct Tap {
  V4 u, g0, g1;
};

YHA_HD int   bits_of(float f) { int i; __builtin_memcpy(&i, &f, 4); return i; }
YHA_HD float float_of(int i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
YHA_HD bool  finite_(float f) { return (bits_of(f) & 0x7f800000) != 0x7f800000; }

// the effective albedo of one channel
YHA_HD float effective_albedo(float a) { return (a < 1e-3f) ? 1.0f : a; }
// ... of a pixel: 1 on a miss, 1 without demodulation (albedo NULL)
YHA_HD void pixel_albedo(const float* albedo, size_t pix, int id, float eff[3]) {
  for (int k = 0; k < 3; k++) eff[k] = (albedo && id != -1) ? effective_albedo(albedo[3 * pix + k]) : 1.0f;
}

// What the pack step makes of one pixel: c = its colour (already resolved), the planes NULL where the parameters do not need them.
YHA_HD Tap pack_pixel(V4 c, size_t pix, const int* object, const float* normal, const float* position, const float* albedo) {
  const int id = object[pix];
  float     eff[3];
  pixel_albedo(albedo, pix, id, eff);
  Tap t;
  t.u  = V4{c.x / eff[0], c.y / eff[1], c.z / eff[2], c.w};
  t.g0 = normal ? V4{normal[3 * pix], normal[3 * pix + 1], normal[3 * pix + 2], float_of(id)} : V4{0, 0, 0, float_of(id)};
  t.g1 = position ? V4{position[3 * pix], position[3 * pix + 1], position[3 * pix + 2], 0} : V4{0, 0, 0, 0};
  return t;
}

YHA_HD float dist2(V4 a, V4 b) {
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return dx * dx + dy * dy + dz * dz;
}

// One level at pixel (px, py): fetch(qx, qy) returns the Tap of a pixel INSIDE the image. 25 taps, dy outer, dx inner, one float
// accumulator per channel and one for the weights, summed in tap order; a tap of weight 0 is not added.
template <class Fetch>
YHA_HD V4 level_pixel(const Fetch& fetch, int px, int py, int width, int height, int level, const yh_denoise_params& P) {
  const Tap c   = fetch(px, py);
  const int idp = bits_of(c.g0.w);
  if (idp == -1) return c.u;
  const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const int   s       = 1 << level;
  const float sn2 = P.sigma_normal * P.sigma_normal, sx2 = P.sigma_position * P.sigma_position;
  const float scl = P.sigma_color * (1.0f / (float)s), sc2 = scl * scl;
  float       acc[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = py + s * dy;
    if (qy < 0 || qy >= height) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = px + s * dx;
      if (qx < 0 || qx >= width) continue;
      const Tap q = fetch(qx, qy);
      if (P.match_object && bits_of(q.g0.w) != idp) continue;
      if (!finite_(q.u.x) || !finite_(q.u.y) || !finite_(q.u.z)) continue;
      const float h  = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy];
      const float xn = P.sigma_normal > 0 ? dist2(c.g0, q.g0) / sn2 : 0.0f;
      const float xx = P.sigma_position > 0 ? dist2(c.g1, q.g1) / sx2 : 0.0f;
      const float xc = P.sigma_color > 0 ? dist2(c.u, q.u) / sc2 : 0.0f;
      const float x  = xn + xx + xc;
      if (!(x >= 0)) continue;
      const float w = h / (1 + x + 0.5f * x * x);
      if (w == 0) continue;
      acc[0] += w * q.u.x, acc[1] += w * q.u.y, acc[2] += w * q.u.z;
      sw += w;
    }
  }
  if (sw == 0 || !finite_(c.u.x) || !finite_(c.u.y) || !finite_(c.u.z)) return c.u;
  return V4{acc[0] / sw, acc[1] / sw, acc[2] / sw, c.u.w};
}

// after the last level: the albedo back
YHA_HD V4 remodulate(V4 u, size_t pix, int id, const float* albedo) {
  float eff[3];
  pixel_albedo(albedo, pix, id, eff);
  return V4{u.x * eff[0], u.y * eff[1], u.z * eff[2], u.w};
}

// whether a parameter set is one the entry points take
YHA_HD bool params_ok(const yh_denoise_params& P) { return P.iterations >= 0 && P.iterations <= YH_DENOISE_MAX_ITERATIONS; }

}  // namespace yha
#endif
