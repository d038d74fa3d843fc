// image_planes.h — the planes of yh_gbuffer (include/yhair.h: the first-hit feature pass), stated once: their names, order and bytes per
// pixel, which of them a stage of the image passes reads, and which one a caller left out. gbuffer.cpp writes them, denoise.cpp and
// temporal.cpp read them, image_pass.cpp allocates and stages them — all by name, through this header. No HIP call, no context, no
// allocation: plain C++ over the two parameter structs.
#ifndef YH_IMAGE_PLANES_H_
#define YH_IMAGE_PLANES_H_
#include <stddef.h>
#include <string.h>

#include "yhair.h"

// name, bytes per pixel — in the order of yh_gbuffer's members
#define YH_PLANES(X) \
  X(object, 4) X(element, 4) X(material, 4) X(uv, 8) X(distance, 4) X(position, 12) X(normal, 12) X(tangent, 12) X(texcoord, 8) X(albedo, 12) X(ray, 24)

enum Plane {
#define X(name, bytes) PLANE_##name,
  YH_PLANES(X)
#undef X
  PLANES
};
#define X(name, bytes) bytes,
constexpr size_t plane_bytes[PLANES] = {YH_PLANES(X)};
#undef X
#define X(name, bytes) #name,
constexpr const char* plane_name[PLANES] = {YH_PLANES(X)};
#undef X
#define X(name, bytes) static_assert(offsetof(yh_gbuffer, name) == PLANE_##name * sizeof(void*), "yh_gbuffer's planes in the order of YH_PLANES");
YH_PLANES(X)
#undef X
static_assert(sizeof(yh_gbuffer) == PLANES * sizeof(void*), "yh_gbuffer is its planes and nothing else");

// plane k of a yh_gbuffer, whatever its element type
inline void* plane_of(const yh_gbuffer& g, int k) {
  void* p;
  memcpy(&p, (const char*)&g + (size_t)k * sizeof(void*), sizeof(p));
  return p;
}
inline void set_plane(yh_gbuffer& g, int k, void* p) { memcpy((char*)&g + (size_t)k * sizeof(void*), &p, sizeof(p)); }

// ---- sets of planes, one bit each ----
constexpr unsigned plane_bit(Plane k) { return 1u << k; }
inline unsigned    planes_present(const yh_gbuffer& g) {
  unsigned mask = 0;
  for (int k = 0; k < PLANES; k++)
    if (plane_of(g, k)) mask |= 1u << k;
  return mask;
}
// what the a-trous filter reads under `p` (NULL or no iteration: it does not run, nothing). A plane that is given but not read is dropped
// (planes_in), so that it changes nothing.
inline unsigned filter_planes(const yh_denoise_params* p) {
  if (!p || p->iterations <= 0) return 0;
  return plane_bit(PLANE_object) | (p->sigma_normal > 0 ? plane_bit(PLANE_normal) : 0) | (p->sigma_position > 0 ? plane_bit(PLANE_position) : 0) |
         (p->demodulate ? plane_bit(PLANE_albedo) : 0);
}
// ... the temporal step, and yh_temporal_display's one feature pass for both
constexpr unsigned temporal_planes() { return plane_bit(PLANE_object) | plane_bit(PLANE_position); }
inline unsigned    display_planes(const yh_denoise_params* p) { return temporal_planes() | filter_planes(p); }
// ... the variance stage (include/yhair.h: VARIANCE). Stage M and S (p NULL: the plain temporal step): the temporal planes and, where
// `demodulate` is set, the albedo. Stage F: what the a-trous filter reads under the same parameters. yh_svgf_display: one feature pass for all.
inline unsigned moment_planes(const yh_variance_params* p) { return temporal_planes() | (p && p->demodulate ? plane_bit(PLANE_albedo) : 0); }
inline unsigned variance_filter_planes(const yh_variance_params* p) {
  if (!p || p->iterations <= 0) return 0;
  return plane_bit(PLANE_object) | (p->sigma_normal > 0 ? plane_bit(PLANE_normal) : 0) | (p->sigma_position > 0 ? plane_bit(PLANE_position) : 0) |
         (p->demodulate ? plane_bit(PLANE_albedo) : 0);
}
inline unsigned svgf_planes(const yh_variance_params* p) { return moment_planes(p) | variance_filter_planes(p); }

// The guide planes in the order the refusals name them and the passes allocate them.
constexpr Plane guide_order[4] = {PLANE_object, PLANE_normal, PLANE_position, PLANE_albedo};
// the first plane of `mask` (a set of guide planes) that `g` lacks, by name; NULL: none
inline const char* missing_plane(unsigned mask, const yh_gbuffer& g) {
  for (Plane k : guide_order)
    if ((mask & plane_bit(k)) && !plane_of(g, k)) return plane_name[k];
  return nullptr;
}
// `g` with the planes outside `mask` dropped
inline yh_gbuffer planes_in(unsigned mask, const yh_gbuffer& g) {
  yh_gbuffer r{};
  for (int k = 0; k < PLANES; k++)
    if (mask & (1u << k)) set_plane(r, k, plane_of(g, k));
  return r;
}
// the four guide planes of the unit-level entries, which only read them, as a yh_gbuffer
inline yh_gbuffer guides_of(const int* object, const float* normal, const float* position, const float* albedo) {
  yh_gbuffer g{};
  g.object = const_cast<int*>(object), g.normal = const_cast<float*>(normal), g.position = const_cast<float*>(position), g.albedo = const_cast<float*>(albedo);
  return g;
}
#endif
