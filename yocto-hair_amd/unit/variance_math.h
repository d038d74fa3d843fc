// variance_math.h — the arithmetic of the variance stage (include/yhair.h: VARIANCE; the variance estimate of SVGF, Schied et al. 2017), for
// BOTH sides: the host library (g++, host/variance.cpp) and the device (hipcc, unit/variance.hip). One text; + - x / and comparisons only,
// no libm call, and neither build contracts a multiply and an add (-ffp-contract=off on the device, no FMA in the x86-64 baseline), so both
// give the same bits, as unit/atrous_math.h and unit/reproject_math.h do. It reuses those two and changes nothing they compute.
//
// Stage M's history of a pixel is TEMPORAL's hc and hg and a third float4, hm = {M1, M2, the steps' bits, vt}. Stage F's pixel is DENOISE's
// three float4 with the variance where the alpha was: u = {working colour rgb, variance}; no tap reads alpha, the last level takes it
// from the caller's image.
#ifndef YH_VARIANCE_MATH_H_
#define YH_VARIANCE_MATH_H_

#include "atrous_math.h"
#include "reproject_math.h"

#ifdef __HIPCC__
#define YHV_HD __host__ __device__ inline
#else
#define YHV_HD inline
#endif

namespace yhv {

using yht::bits_of;
using yht::finite_;
using yht::float_of;
using yht::V4;

struct Moments {
  float m1, m2;
  int   steps;
};
struct ResultM {
  V4      out;
  int     length;
  Moments m;
};

YHV_HD float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
// vt of a pair of moments
YHV_HD float variance_of(float m1, float m2) {
  const float d = m2 - m1 * m1;
  return d > 0 ? d : 0.0f;
}
YHV_HD V4 plane_of(const Moments& m) { return V4{m.m1, m.m2, float_of(m.steps), variance_of(m.m1, m.m2)}; }

// ---- stage M ----
// yht::reproject_pixel with the moments beside the colour: TEMPORAL's steps 1 - 7 in its words and its order — every operation on the colour
// is the one reproject_pixel does, so out and length have its bits — and, wherever the colour takes a tap, the moments take it too.
// eff: the pixel's effective albedo (yha::pixel_albedo). fetch(qx, qy, hc, hg, hm) loads the history of a pixel INSIDE the image;
// have_moments 0: there is no moment history (hm is not read, every tap has steps 0).
template <class Fetch>
YHV_HD ResultM reproject_pixel_m(const Fetch& fetch, int i, int j, int W, int H, V4 c, const float eff[3], int id, F3 x, int n, const float* cam,
    const float* pcam, bool same_camera, const yht::Motion& m, const yh_temporal_params& P, bool have_history) {
  using namespace yht;
  // 1. pass-through
  if (id == -1 || !finite_(c.x) || !finite_(c.y) || !finite_(c.z)) return ResultM{c, 0, Moments{0.0f, 0.0f, 0}};
  const float   l = lum(c.x / eff[0], c.y / eff[1], c.z / eff[2]);
  const ResultM fresh{c, n, Moments{l, l * l, 1}};
  if (!have_history) return fresh;
  // 2. the previous world position
  F3   y     = x;
  bool still = true;
  if (m.cur && id >= 0 && id < m.count) {
    if (m.usable && m.usable[id] == 0) return fresh;
    const float* fc = m.cur + (size_t)id * m.stride;
    const float* fp = m.prev + (size_t)id * 12;
    if (!same_bits(fc, fp, 12)) {
      y     = transform_point(fp, transform_point(m.cur_inv + (size_t)id * m.stride, x));
      still = false;
    }
  }
  // 3. projection into the previous camera
  float fx, fy;
  if (!project(pcam, y, W, H, fx, fy)) return fresh;
  if (!finite_(fx) || !finite_(fy) || !(-1.0f < fx && fx < (float)W) || !(-1.0f < fy && fy < (float)H)) return fresh;
  // 4. taps
  int   qx[4], qy[4], ntaps;
  float w[4];
  if (same_camera && still) {
    qx[0] = i, qy[0] = j, w[0] = 1.0f, ntaps = 1;
  } else {
    const int   i0 = floor_(fx), j0 = floor_(fy);
    const float tx = fx - (float)i0, ty = fy - (float)j0;
    qx[0] = i0, qy[0] = j0, w[0] = (1.0f - tx) * (1.0f - ty);
    qx[1] = i0 + 1, qy[1] = j0, w[1] = tx * (1.0f - ty);
    qx[2] = i0, qy[2] = j0 + 1, w[2] = (1.0f - tx) * ty;
    qx[3] = i0 + 1, qy[3] = j0 + 1, w[3] = tx * ty;
    ntaps = 4;
  }
  // 5., 6. the valid taps, summed in tap order
  const float s2     = P.sigma_position * P.sigma_position;
  float       acc[3] = {0.0f, 0.0f, 0.0f}, am[2] = {0.0f, 0.0f}, S = 0.0f;
  int         N = 0x7fffffff, T = 0x7fffffff;
  for (int k = 0; k < ntaps; k++) {
    if (qx[k] < 0 || qx[k] >= W || qy[k] < 0 || qy[k] >= H) continue;
    V4 hc, hg, hm;
    fetch(qx[k], qy[k], hc, hg, hm);
    const int len = bits_of(hc.w);
    if (!(len > 0)) continue;
    if (P.match_object && bits_of(hg.w) != id) continue;
    if (!finite_(hc.x) || !finite_(hc.y) || !finite_(hc.z)) continue;
    if (P.sigma_position > 0) {
      const F3 e = y - F3{hg.x, hg.y, hg.z};
      if (!(dot(e, e) <= s2)) continue;
    }
    if (w[k] == 0) continue;
    acc[0] += w[k] * hc.x, acc[1] += w[k] * hc.y, acc[2] += w[k] * hc.z;
    am[0] += w[k] * hm.x, am[1] += w[k] * hm.y;
    S += w[k];
    N = (len < N) ? len : N;
    const int st = bits_of(hm.z);
    T            = (st < T) ? st : T;
  }
  if (!(S > 0)) return fresh;
  N = (N < P.max_history) ? N : P.max_history;
  // 7. blend
  const float h[3] = {acc[0] / S, acc[1] / S, acc[2] / S};
  const float a    = (float)n / (float)(N + n);
  ResultM     r{V4{h[0] + (c.x - h[0]) * a, h[1] + (c.y - h[1]) * a, h[2] + (c.z - h[2]) * a, c.w}, N + n, fresh.m};
  const float hm1 = am[0] / S, hm2 = am[1] / S;
  if (T > 0 && finite_(hm1) && finite_(hm2)) {
    r.m.m1    = hm1 + (fresh.m.m1 - hm1) * a;
    r.m.m2    = hm2 + (fresh.m.m2 - hm2) * a;
    r.m.steps = ((T < YH_VARIANCE_MAX_STEPS - 1) ? T : YH_VARIANCE_MAX_STEPS - 1) + 1;
  }
  return r;
}

// ---- stage S ----
#define YH_VAR_WINDOW 3 /* the 7 x 7 window's radius */
// whether pixel (steps) looks at its neighbours at all
YHV_HD bool spatial_needed(int steps, int min_steps) { return steps > 0 && steps < min_steps; }
// One pixel: fetch(qx, qy, hm, hg) loads stage M's planes of a pixel INSIDE the image; it is called for a neighbour only where
// spatial_needed holds.
template <class Fetch>
YHV_HD float spatial_pixel(const Fetch& fetch, int px, int py, int W, int H, const yh_temporal_params& P, int min_steps) {
  V4 cm, cg;
  fetch(px, py, cm, cg);
  const int   steps = bits_of(cm.z);
  const float vt    = variance_of(cm.x, cm.y);
  if (steps >= min_steps) return vt;
  if (!(steps > 0)) return 0.0f;
  const int   id = bits_of(cg.w);
  const float s2 = P.sigma_position * P.sigma_position;
  float       a1 = 0.0f, a2 = 0.0f;
  int         k  = 0;
  for (int dy = -YH_VAR_WINDOW; dy <= YH_VAR_WINDOW; dy++) {
    const int qy = py + dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -YH_VAR_WINDOW; dx <= YH_VAR_WINDOW; dx++) {
      const int qx = px + dx;
      if (qx < 0 || qx >= W) continue;
      V4 qm, qg;
      fetch(qx, qy, qm, qg);
      if (!(bits_of(qm.z) > 0)) continue;
      if (P.match_object && bits_of(qg.w) != id) continue;
      if (P.sigma_position > 0) {
        const F3 e = F3{cg.x, cg.y, cg.z} - F3{qg.x, qg.y, qg.z};
        if (!(dot(e, e) <= s2)) continue;
      }
      if (!finite_(qm.x) || !finite_(qm.y)) continue;
      a1 += qm.x, a2 += qm.y;
      k++;
    }
  }
  if (k == 0) return vt;
  const float kf = (float)k, A1 = a1 / kf, A2 = a2 / kf;
  const float e  = A2 - A1 * A1;
  const float vs = e > 0 ? e : 0.0f;
  return vt > vs ? vt : vs;
}

// ---- stage F ----
// What the pack step makes of one pixel: yha::pack_pixel with the variance in u.w.
YHV_HD yha::Tap pack_pixel(yha::V4 c, float v, size_t pix, const int* object, const float* normal, const float* position, const float* albedo) {
  yha::Tap t = yha::pack_pixel(c, pix, object, normal, position, albedo);
  t.u.w      = v;
  return t;
}

// g of pixel (px, py): the variance through the 3 x 3 kernel at spacing 1
template <class Fetch>
YHV_HD float prefilter_variance(const Fetch& fetch, int px, int py, int width, int height, int idp, int match_object) {
  const float k3[3] = {1.0f / 4.0f, 1.0f / 8.0f, 1.0f / 16.0f};
  float       sv = 0.0f, sk = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = py + dy;
    if (qy < 0 || qy >= height) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = px + dx;
      if (qx < 0 || qx >= width) continue;
      const yha::Tap q = fetch(qx, qy);
      if (match_object && yha::bits_of(q.g0.w) != idp) continue;
      if (!finite_(q.u.w)) continue;
      const float k = k3[(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)];
      sv += k * q.u.w;
      sk += k;
    }
  }
  return sk > 0 ? sv / sk : 0.0f;
}

// One level at pixel (px, py): yha::level_pixel with the luminance term scaled by g in the place of the colour term, and the variance
// filtered by the squared weights. fetch(qx, qy) returns the Tap of a pixel INSIDE the image. The result's w is v'.
template <class Fetch>
YHV_HD yha::V4 level_pixel(const Fetch& fetch, int px, int py, int width, int height, int level, const yh_variance_params& P) {
  using namespace yha;
  const Tap c   = fetch(px, py);
  const int idp = yha::bits_of(c.g0.w);
  if (idp == -1) return c.u;
  const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const int   s       = 1 << level;
  const float sn2 = P.sigma_normal * P.sigma_normal, sx2 = P.sigma_position * P.sigma_position;
  const float g   = prefilter_variance(fetch, px, py, width, height, idp, P.match_object);
  const float sl2 = (P.sigma_luminance * P.sigma_luminance) * g + P.epsilon;
  const float lp  = lum(c.u.x, c.u.y, c.u.z);
  float       acc[3] = {0.0f, 0.0f, 0.0f}, av = 0.0f, sw = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = py + s * dy;
    if (qy < 0 || qy >= height) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = px + s * dx;
      if (qx < 0 || qx >= width) continue;
      const Tap q = fetch(qx, qy);
      if (P.match_object && yha::bits_of(q.g0.w) != idp) continue;
      if (!finite_(q.u.x) || !finite_(q.u.y) || !finite_(q.u.z) || !finite_(q.u.w)) continue;
      const float h  = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy];
      const float xn = P.sigma_normal > 0 ? dist2(c.g0, q.g0) / sn2 : 0.0f;
      const float xx = P.sigma_position > 0 ? dist2(c.g1, q.g1) / sx2 : 0.0f;
      const float dl = lp - lum(q.u.x, q.u.y, q.u.z);
      const float xl = P.sigma_luminance > 0 ? (dl * dl) / sl2 : 0.0f;
      const float x  = xn + xx + xl;
      if (!(x >= 0)) continue;
      const float w = h / (1 + x + 0.5f * x * x);
      if (w == 0) continue;
      acc[0] += w * q.u.x, acc[1] += w * q.u.y, acc[2] += w * q.u.z;
      av += (w * w) * q.u.w;
      sw += w;
    }
  }
  if (sw == 0 || !finite_(c.u.x) || !finite_(c.u.y) || !finite_(c.u.z)) return c.u;
  return yha::V4{acc[0] / sw, acc[1] / sw, acc[2] / sw, av / (sw * sw)};
}

// whether a parameter set is one the entry points take
YHV_HD bool params_ok(const yh_variance_params& P) {
  return P.iterations >= 0 && P.iterations <= YH_DENOISE_MAX_ITERATIONS && P.min_steps >= 1 && P.epsilon > 0;
}

}  // namespace yhv
#endif
