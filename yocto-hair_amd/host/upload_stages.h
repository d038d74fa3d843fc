// upload_stages.h — the stages of yh_upload_scene (scene_upload.cpp) that make no HIP call and need no context: pure functions over the
// description and plain vectors, so that a g++-only program can run them (tests/cpp/test_upload_stages.cpp). One object's row, the
// environments' rows, the light values from the arrays the caller lent (the edits compute theirs on the device, unit/light_list.hip: the
// edit tests compare the two), the texture conversion, and the description bytes the fingerprint mixes. A refusal travels out as a code;
// the upload turns it into its message, as it does for light_layout.h and blob_layout.h.
#ifndef YH_UPLOAD_STAGES_H_
#define YH_UPLOAD_STAGES_H_
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../csrc/yh_device.h"
#include "../unit/light_math.h"   // triangle_area: an area light's cdf entry, shared with the device
#include "../unit/object_math.h"  // inverse_frame, padded_world_box: shared with the device
#include "bvh_build.h"
#include "light_layout.h"
#include "parallel_for.h"
#include "yhair.h"

#pragma GCC visibility push(hidden)  // internal to libyhair.so
// ---- objects ---------------------------------------------------------------------------------------------------------------------------
// what an object's row takes from its shape: the kind, where the shape's arrays begin, and its regions of the traversal array (32-byte units)
struct ObjectShape {
  int       kind, prim_base, vert_base, elem_base, has_normals, has_texcoords;
  long long test_off, node_off[3];
};
inline void object_row(const yh_object& o, const ObjectShape& s, const yhh::Box& world_box, yhd_object& d) {
  memset(&d, 0, sizeof(d));
  memcpy(d.frame, o.frame, 48);
  inverse_frame(o.frame, true, d.inv_frame);
  d.kind = s.kind, d.node_base = 0, d.prim_base = s.prim_base, d.vert_base = s.vert_base;
  d.elem_base = s.elem_base, d.has_normals = s.has_normals, d.material = o.material, d.has_texcoords = s.has_texcoords;
  d.lane_root = (int)s.node_off[0], d.lane_test = (int)s.test_off, d.lane_root8 = (int)s.node_off[1], d.lane_root16 = (int)s.node_off[2];
  padded_world_box(world_box.min, world_box.max, d.wbox_min, d.wbox_max);
}

// ---- environments ----------------------------------------------------------------------------------------------------------------------
// rows[YH_MAX_ENVS] and the texels of the textured ones one behind the other; emission (3 floats each) and texel_count: light_layout's inputs
inline void environment_rows(const yh_scene_desc& sd, yhd_environment* rows, std::vector<yhd_float4>& texels, float* emission, int* texel_count) {
  for (int ei = 0; ei < sd.num_environments; ei++) {
    const yh_environment& e = sd.environments[ei];
    yhd_environment&      d = rows[ei];
    memcpy(d.frame, e.frame, 48);
    inverse_frame(e.frame, false, d.inv_frame);
    memcpy(d.emission, e.emission, 12);
    d.tex_w = e.texels ? e.tex_width : 0, d.tex_h = e.texels ? e.tex_height : 0;
    d.texel_base = (int)texels.size();
    if (e.texels)
      for (size_t t = 0; t < (size_t)e.tex_width * e.tex_height; t++) texels.push_back({e.texels[3 * t], e.texels[3 * t + 1], e.texels[3 * t + 2], 0});
    memcpy(emission + 3 * ei, e.emission, 12);
    texel_count[ei] = e.texels ? (int)((size_t)e.tex_width * e.tex_height) : 0;
  }
}

// ---- the lights' values (init_lights, pt.cpp:1695-1740); which lights there are and where their entries sit: light_layout.h ----------------
// the texel cdf of a textured environment (pt.cpp:1720-1734, the host's sine), `stride` floats per texel, appended to `cdf` as one float
// chain (the light edits run it too, over the texels they read back: light_edit.cpp)
inline void append_env_cdf(const float* texels, int stride, int width, int height, std::vector<float>& cdf) {
  const float  pi = (float)3.14159265358979323846;
  const size_t n = (size_t)width * height, at = cdf.size();
  for (size_t i = 0; i < n; i++) {
    int   iy    = (int)(i / width);
    float th    = (iy + 0.5f) * pi / height;
    float mx    = fmax_(fmax_(texels[stride * i], texels[stride * i + 1]), texels[stride * i + 2]);
    float value = mx * std::sin(th);
    if (i) value += cdf[at + i - 1];
    cdf.push_back(value);
  }
}
// every light's segment, in list order: an area cdf by element (one float chain in element order), or a texel cdf
inline void light_cdfs(const yh_scene_desc& sd, const LightLayout& lights, std::vector<float>& cdf) {
  for (int li = 0; li < lights.num_lights; li++) {
    const yhd_light& L = lights.lights[li];
    if (L.object >= 0) {
      const yh_shape& s = sd.shapes[sd.objects[L.object].shape];
      for (int t = 0; t < s.num_triangles; t++) {
        float area = triangle_area(ld3(s.positions + 3 * (size_t)s.triangles[3 * t]), ld3(s.positions + 3 * (size_t)s.triangles[3 * t + 1]),
            ld3(s.positions + 3 * (size_t)s.triangles[3 * t + 2]));  // (unit/light_math.h: triangle_area, math.h:3306)
        if (t) area += cdf.back();
        cdf.push_back(area);
      }
    } else if (L.cdf_count > 0) {
      const yh_environment& e = sd.environments[L.environment];
      append_env_cdf(e.texels, 3, e.tex_width, e.tex_height, cdf);
    }
  }
}
// a small area light's record in the table the kernels keep in LDS (yh_device.h) — root box, leaf-ordered triangles, area cdf: everything
// sample_lights / sample_lights_pdf read. rec: the shape's leaf records (6 float4 per triangle); light_cdf: the whole array
inline void small_light_record(const yhd_light& L, const yhh::Box& root, const yhd_float4* rec, const float* light_cdf, std::vector<yhd_float4>& table) {
  yhd_float4 b0{root.min[0], root.min[1], root.min[2], 0}, b1{root.max[0], root.max[1], root.max[2], light_cdf[(size_t)L.cdf_base + L.cdf_count - 1]};
  memcpy(&b0.w, &L.cdf_count, 4);
  table.push_back(b0), table.push_back(b1);
  for (int t = 0; t < YH_SMALL_LIGHT_TRIS; t++)
    for (int k = 0; k < 3; k++) table.push_back(t < L.cdf_count ? rec[6 * t + k] : yhd_float4{0, 0, 0, 0});
  yhd_float4 cdf{0, 0, 0, 0};
  for (int t = 0; t < L.cdf_count; t++) (&cdf.x)[t] = light_cdf[(size_t)L.cdf_base + t];
  table.push_back(cdf);
}
// coarse index of the first textured environment light's cdf: 2048 entries (8 KB) halve the dependent fetches of its 21-step binary search
inline void coarse_index(const LightLayout& lights, const float* light_cdf, std::vector<float>& tab) {
  if (lights.env_tab_light < 0) return;
  const yhd_light& L = lights.lights[lights.env_tab_light];
  const int n = L.cdf_count, S = lights.env_tab_stride, K = lights.env_tab_k;
  tab.resize((size_t)K);
  for (int k = 0; k < K; k++) tab[(size_t)k] = light_cdf[(size_t)L.cdf_base + (size_t)std::min<int64_t>(n, (int64_t)(k + 1) * S) - 1];
}

// ---- material colour textures (lookup_texture's per-texel conversion done once, pt.cpp:147-164) ---------------------------------------------
// maps: one per material where maps are in force (some material has an effective map), else NULL. *at: the material or the texture a
// refusal names.
enum { YH_TEXTURES_OK = 0, YH_TEXTURES_MISSING, YH_TEXTURES_EMPTY };
inline int convert_textures(const yh_scene_desc& sd, const yh_material_maps* maps, std::vector<yhd_texture>& textures, std::vector<yhd_float4>& tex_texels, int* at) {
  textures.assign((size_t)std::max(0, sd.num_textures), yhd_texture{});
  std::vector<char> need_linear(textures.size(), 0);
  for (int i = 0; i < sd.num_materials; i++) {
    const yh_material& m = sd.materials[i];
    for (int id : {m.emission_tex, m.color_tex, m.scattering_tex})
      if (id < 0 || id > sd.num_textures) return *at = i, YH_TEXTURES_MISSING;
    if (m.emission_tex > 0) need_linear[(size_t)m.emission_tex - 1] = 1;  // transmission *= emission_tex.x, linear (pt.cpp:421)
    if (maps)  // every map is looked up linear (pt.cpp:413-424, 337)
      for (int id : {maps[i].specular_tex, maps[i].metallic_tex, maps[i].roughness_tex, maps[i].opacity_tex, maps[i].normal_tex})
        if (id > 0) need_linear[(size_t)id - 1] = 1;
  }
  auto srgb_to_rgb = [](float srgb) {  // math.h:3742-3745
    return (srgb <= 0.04045) ? srgb / 12.92f : std::pow((srgb + 0.055f) / (1.0f + 0.055f), 2.4f);
  };
  std::vector<char> used(textures.size(), !maps);  // (with maps: a texture only a transmission map names is not uploaded)
  if (maps)
    for (int i = 0; i < sd.num_materials; i++) {
      const yh_material& m = sd.materials[i];
      for (int id : {m.emission_tex, m.color_tex, m.scattering_tex})
        if (id > 0) used[(size_t)id - 1] = 1;
    }
  for (size_t t = 0; t < textures.size(); t++) used[t] = used[t] || need_linear[t];
  for (size_t t = 0; t < textures.size(); t++) {
    const yh_texture& src = sd.textures[t];
    if (src.width <= 0 || src.height <= 0 || !src.pixels) return *at = (int)t, YH_TEXTURES_EMPTY;
    size_t       n = (size_t)src.width * src.height;
    yhd_texture& d = textures[t];
    d.width = src.width, d.height = src.height, d.srgb_base = (int)tex_texels.size(), d.linear_base = -1;
    if (!used[t]) {
      d.srgb_base = -1;
      continue;
    }
    tex_texels.resize(tex_texels.size() + n);
    yhd_float4* out = tex_texels.data() + d.srgb_base;
    if (src.is_byte) {
      auto b = (const unsigned char*)src.pixels;
      parallel_for((int)n, [&](int i) {
        out[i] = {srgb_to_rgb(b[3 * (size_t)i] / 255.0f), srgb_to_rgb(b[3 * (size_t)i + 1] / 255.0f), srgb_to_rgb(b[3 * (size_t)i + 2] / 255.0f), 0};
      });
      if (need_linear[t]) {
        d.linear_base = (int)tex_texels.size();
        tex_texels.resize(tex_texels.size() + n);
        yhd_float4* lin = tex_texels.data() + d.linear_base;
        parallel_for((int)n, [&](int i) { lin[i] = {b[3 * (size_t)i] / 255.0f, b[3 * (size_t)i + 1] / 255.0f, b[3 * (size_t)i + 2] / 255.0f, 0}; });
      }
    } else {
      auto f = (const float*)src.pixels;
      parallel_for((int)n, [&](int i) { out[i] = {f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2], 0}; });
      d.linear_base = d.srgb_base;
    }
  }
  return YH_TEXTURES_OK;
}

// ---- the bytes of the description that the scene's fingerprint mixes, in the fingerprint's order (scene_fingerprint) -------------------------
// geometry: the object rows, then per shape its three counts and its first and last 256 positions (key_positions[shape]: where those begin,
// for the shape edits); envs: every environment's head
inline void description_key_bytes(const yh_scene_desc& sd, std::vector<unsigned char>& geometry, std::vector<unsigned char>& envs, std::vector<size_t>& key_positions) {
  auto bytes = [](std::vector<unsigned char>& to, const void* p, size_t n) { to.insert(to.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
  geometry.clear(), envs.clear(), key_positions.clear();
  bytes(geometry, sd.objects, sizeof(yh_object) * (size_t)sd.num_objects);
  for (int i = 0; i < sd.num_shapes; i++) {
    const yh_shape& sh = sd.shapes[i];
    int counts[3] = {sh.num_vertices, sh.num_lines, sh.num_triangles};
    bytes(geometry, counts, sizeof(counts));
    key_positions.push_back(geometry.size());
    if (sh.positions && sh.num_vertices > 0) {
      const size_t n = (size_t)sh.num_vertices, take = std::min<size_t>(n, 256);
      bytes(geometry, sh.positions, take * 12), bytes(geometry, sh.positions + 3 * (n - take), take * 12);
    }
  }
  for (int i = 0; i < sd.num_environments; i++) bytes(envs, &sd.environments[i], offsetof(yh_environment, texels));
}
#pragma GCC visibility pop
#endif
