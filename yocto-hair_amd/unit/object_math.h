// object_math.h — what an object's frame turns into, for BOTH sides: the host library (g++, through host/context_internal.h: the upload's
// object section) and the device (hipcc, unit/objects.hip: yh_update_objects). One text, the reference's operation order, and neither build
// contracts a multiply and an add (-ffp-contract=off on the device, no FMA in the x86-64 baseline), so both give the same bits.
#ifndef YH_OBJECT_MATH_H_
#define YH_OBJECT_MATH_H_

#ifdef __HIPCC__
#define YH_HD __host__ __device__
#else
#define YH_HD
#endif

namespace {

// ---- tiny vector helpers with the reference's operation order --------
struct F3 {
  float x, y, z;
};
YH_HD F3    operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
YH_HD F3    operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
YH_HD F3    operator-(F3 a) { return {-a.x, -a.y, -a.z}; }
YH_HD F3    operator*(F3 a, float b) { return {a.x * b, a.y * b, a.z * b}; }
YH_HD float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
YH_HD F3    cross(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
YH_HD float fmin_(float a, float b) { return (a < b) ? a : b; }
YH_HD float fmax_(float a, float b) { return (a > b) ? a : b; }
YH_HD F3    ld3(const float* p) { return {p[0], p[1], p[2]}; }
YH_HD void  st3(float* p, F3 a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

// inverse(frame, non_rigid = true) (math.h:2877-2885, 2721-2741)
YH_HD void inverse_frame(const float* f, bool non_rigid, float* out) {
  F3 x = ld3(f), y = ld3(f + 3), z = ld3(f + 6), o = ld3(f + 9);
  F3 rx, ry, rz;
  if (non_rigid) {
    F3    c0 = cross(y, z), c1 = cross(z, x), c2 = cross(x, y);
    float det = dot(x, cross(y, z));
    float s   = 1 / det;
    rx = F3{c0.x, c1.x, c2.x} * s, ry = F3{c0.y, c1.y, c2.y} * s, rz = F3{c0.z, c1.z, c2.z} * s;
  } else {
    rx = {x.x, y.x, z.x}, ry = {x.y, y.y, z.y}, rz = {x.z, y.z, z.z};
  }
  F3 ro = -(rx * o.x + ry * o.y + rz * o.z);
  st3(out, rx), st3(out + 3, ry), st3(out + 6, rz), st3(out + 9, ro);
}
YH_HD F3 transform_point(const float* f, F3 b) {
  return ld3(f) * b.x + ld3(f + 3) * b.y + ld3(f + 6) * b.z + ld3(f + 9);
}

// transform_bbox (math.h:3174-3185): the box of the eight transformed corners of {bmin, bmax}
YH_HD void transform_bbox(const float* frame, const float* bmin, const float* bmax, float* lo, float* hi) {
  lo[0] = lo[1] = lo[2] = 3.402823466e+38f, hi[0] = hi[1] = hi[2] = -3.402823466e+38f;  // numeric_limits<float>::max() / lowest()
  for (int c = 0; c < 8; c++) {
    F3 corner = {(c & 4) ? bmax[0] : bmin[0], (c & 2) ? bmax[1] : bmin[1], (c & 1) ? bmax[2] : bmin[2]};
    F3 t      = transform_point(frame, corner);
    float tv[3] = {t.x, t.y, t.z};
    for (int k = 0; k < 3; k++) lo[k] = fmin_(lo[k], tv[k]), hi[k] = fmax_(hi[k], tv[k]);
  }
}
// an object's world box with a margin a thousand times the rounding of either box test (yhd_object::wbox_min / wbox_max)
YH_HD void padded_world_box(const float* lo, const float* hi, float* wbox_min, float* wbox_max) {
  float ext = fmax_(fmax_(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
  float eps = 1e-3f * ext + 1e-5f;
  for (int k = 0; k < 3; k++) wbox_min[k] = lo[k] - eps, wbox_max[k] = hi[k] + eps;
  wbox_min[3] = wbox_max[3] = 0;
}

}  // namespace
#endif
