// reproject_math.h — the arithmetic of the temporal stage (include/yhair.h: TEMPORAL; the reprojection of SVGF, Schied et al. 2017), for
// BOTH sides: the host library (g++, host/temporal.cpp: yh_reproject) and the device (hipcc, unit/reproject.hip). One text; + - x / and
// comparisons only, no libm call, and neither build contracts a multiply and an add (-ffp-contract=off on the device, no FMA in the
// x86-64 baseline), so both give the same bits, as unit/atrous_math.h and unit/object_math.h do.
//
// The history of a pixel is two float4: hc = {accumulated rgb, the length's bits}, hg = {world position, the object id's bits}. A camera is
// the 17 floats of yh_camera: frame (x, y, z axes, origin), lens, film x, film y, focus, aperture.
#ifndef YH_REPROJECT_MATH_H_
#define YH_REPROJECT_MATH_H_

#include <stddef.h>

#include "yhair.h"
#include "object_math.h"  // F3, dot, transform_point: the helpers the object rows are made with

#ifdef __HIPCC__
#define YHT_HD __host__ __device__ inline
#else
#define YHT_HD inline
#endif

namespace yht {

struct V4 {
  float x, y, z, w;
};
struct Camera {
  float f[17];
};
// The objects' motion: row `id` of `cur` / `cur_inv` (frame and inverse(frame, non_rigid), `stride` floats apart: the device's object
// rows or a compact copy) and of `prev` (12 floats apart), and `usable`. cur NULL: no motion is given. An id outside [0, count) is
// taken as static and usable, so that no row is read out of bounds.
struct Motion {
  const float *cur, *cur_inv, *prev;
  const int*   usable;
  int          stride, count;
};
struct Result {
  V4  out;
  int length;
};

YHT_HD int   bits_of(float f) { int i; __builtin_memcpy(&i, &f, 4); return i; }
YHT_HD float float_of(int i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
YHT_HD bool  finite_(float f) { return (bits_of(f) & 0x7f800000) != 0x7f800000; }
YHT_HD bool  same_bits(const float* a, const float* b, int n) {
  for (int k = 0; k < n; k++)
    if (bits_of(a[k]) != bits_of(b[k])) return false;
  return true;
}
YHT_HD int floor_(float f) {  // of a finite f inside the int range
  const int i = (int)f;
  return ((float)i > f) ? i - 1 : i;
}

// Step 3: where world point y falls in camera `cam`'s image of W x H pixels, in pixel units (pixel i's centre is fx = i) — the inverse
// of the centre-mode ray of unit/gbuffer.hip (sample_camera_lane at uv + 0.5 with the lens point at zero). false: behind the camera.
YHT_HD bool project(const float* cam, F3 y, int W, int H, float& fx, float& fy) {
  const F3    d  = y - ld3(cam + 9);
  const float lx = dot(d, ld3(cam)), ly = dot(d, ld3(cam + 3)), lz = dot(d, ld3(cam + 6));
  if (!(lz < 0)) return false;
  const float u = 0.5f - (cam[12] * lx) / (cam[13] * lz);
  const float v = 0.5f + (cam[12] * ly) / (cam[14] * lz);
  fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
  return true;
}

// One pixel (i, j): c its colour with n samples in it, id and x its object and world position; fetch(qx, qy, hc, hg) loads the history of
// a pixel INSIDE the image. have_history 0: there is none at all (the first frame) and fetch is never called. same_camera: pcam has
// cam's bits. The result's colour and length, with id and x, are the pixel's new history.
template <class Fetch>
YHT_HD Result reproject_pixel(const Fetch& fetch, int i, int j, int W, int H, V4 c, int id, F3 x, int n, const float* cam, const float* pcam,
    bool same_camera, const Motion& m, const yh_temporal_params& P, bool have_history) {
  // 1. pass-through
  if (id == -1 || !finite_(c.x) || !finite_(c.y) || !finite_(c.z)) return Result{c, 0};
  const Result fresh{c, n};
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
  float       acc[3] = {0.0f, 0.0f, 0.0f}, S = 0.0f;
  int         N = 0x7fffffff;
  for (int k = 0; k < ntaps; k++) {
    if (qx[k] < 0 || qx[k] >= W || qy[k] < 0 || qy[k] >= H) continue;
    V4 hc, hg;
    fetch(qx[k], qy[k], hc, hg);
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
    S += w[k];
    N = (len < N) ? len : N;
  }
  if (!(S > 0)) return fresh;
  N = (N < P.max_history) ? N : P.max_history;
  // 7. blend
  const float h[3] = {acc[0] / S, acc[1] / S, acc[2] / S};
  const float a    = (float)n / (float)(N + n);
  return Result{V4{h[0] + (c.x - h[0]) * a, h[1] + (c.y - h[1]) * a, h[2] + (c.z - h[2]) * a, c.w}, N + n};
}

// whether a parameter set and a sample count are ones the entry points take (N + n stays an int)
YHT_HD bool params_ok(const yh_temporal_params& P) { return P.max_history >= 1 && P.max_history <= (1 << 30); }
YHT_HD bool samples_ok(int n) { return n >= 1 && n <= (1 << 30); }

}  // namespace yht
#endif
