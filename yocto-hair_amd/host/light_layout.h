// light_layout.h — the rule that makes the light list (init_lights, pt.cpp:1695-1740), stated once: which objects and environments are
// lights, in which order, and where each one's entries sit. yh_upload_scene (scene_upload.cpp) and the light edits (light_edit.cpp:
// stage_lights) both call it and fill the arrays it lays out, each in its own way; every light edit is tested bit for bit against a
// fresh upload, so the two must agree on every row. No HIP call, no context, no allocation: plain C++ over the description.
#ifndef YH_LIGHT_LAYOUT_H_
#define YH_LIGHT_LAYOUT_H_
#include <stddef.h>

#include "../csrc/yh_device.h"
#include "yhair.h"

#pragma GCC visibility push(hidden)  // internal to libyhair.so
struct LightShape {
  bool lines;      // a line shape never becomes a light
  int  num_prims;  // its triangles otherwise (0: no light either)
};

struct LightLayoutIn {
  int                num_objects;
  const yh_object*   objects;    // shape and material per object
  const yh_material* materials;  // the whole table: emission
  const LightShape*  shapes;
  int                num_environments;
  const float*       emission;   // 3 floats per environment
  const int*         texels;     // per environment: width x height of its texture, 0 for a constant one
};

struct LightLayout {
  int       num_lights = 0;
  yhd_light lights[YH_MAX_LIGHTS] = {};
  bool      big_lights = false;  // some area light is read through memory (more than YH_SMALL_LIGHT_TRIS triangles)
  int       table_f4 = 0;        // float4 of the small lights' records (yhd_scene::light_table)
  int       env_tab_light = -1, env_tab_k = 0, env_tab_stride = 0;  // the coarse index of ONE texel cdf (yhd_scene::env_tab)
  size_t    cdf_total = 0;       // entries of light_cdf
};

enum { YH_LIGHTS_OK = 0, YH_LIGHTS_OBJECT_TOO_MANY, YH_LIGHTS_ENVIRONMENT_TOO_MANY, YH_LIGHTS_NONE };

inline bool is_black(const float* e) { return e[0] == 0 && e[1] == 0 && e[2] == 0; }

// Objects first, in order, then environments: every object whose material emits and whose shape has triangles is a light of its own (so
// is every instance of an emitter), every environment that emits is one. *at: the object or environment that would be light number
// YH_MAX_LIGHTS + 1, with the two "too many" codes.
inline int light_layout(const LightLayoutIn& in, LightLayout& out, int* at) {
  out = LightLayout{};
  for (int oi = 0; oi < in.num_objects; oi++) {
    const yh_object& o = in.objects[oi];
    if (is_black(in.materials[o.material].emission)) continue;
    const LightShape& s = in.shapes[o.shape];
    if (s.lines || s.num_prims <= 0) continue;
    if (out.num_lights >= YH_MAX_LIGHTS) return *at = oi, YH_LIGHTS_OBJECT_TOO_MANY;
    yhd_light& l = out.lights[out.num_lights++];
    l.object = oi, l.environment = -1, l.cdf_base = (int)out.cdf_total, l.cdf_count = s.num_prims, l.small_base = -1;
    if (s.num_prims <= YH_SMALL_LIGHT_TRIS) l.small_base = out.table_f4, out.table_f4 += YH_SMALL_LIGHT_F4;  // its record in the LDS table
    else out.big_lights = true;
    out.cdf_total += (size_t)s.num_prims;
  }
  for (int ei = 0; ei < in.num_environments; ei++) {
    if (is_black(in.emission + 3 * ei)) continue;
    if (out.num_lights >= YH_MAX_LIGHTS) return *at = ei, YH_LIGHTS_ENVIRONMENT_TOO_MANY;
    yhd_light& l = out.lights[out.num_lights++];
    l.object = -1, l.environment = ei, l.cdf_base = (int)out.cdf_total, l.cdf_count = in.texels[ei], l.small_base = -1;  // (0 texels: no cdf)
    out.cdf_total += (size_t)l.cdf_count;
  }
  if (out.num_lights == 0) return YH_LIGHTS_NONE;
  // the coarse index of the first textured environment light of at least 4096 texels: at most 2048 entries (8 KB), every `stride`-th
  // entry of its cdf, halve the dependent fetches of the binary search over it
  for (int li = 0; li < out.num_lights && out.env_tab_light < 0; li++) {
    const yhd_light& l = out.lights[li];
    if (l.environment < 0 || l.cdf_count < 4096) continue;
    const int n = l.cdf_count, stride = (n + 2047) / 2048;
    out.env_tab_light = li, out.env_tab_k = (n + stride - 1) / stride, out.env_tab_stride = stride;
  }
  return YH_LIGHTS_OK;
}
#pragma GCC visibility pop
#endif
