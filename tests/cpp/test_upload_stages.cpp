// The stages of yh_upload_scene that need no device (yocto-hair_amd/host/upload_stages.h), on a hand-made description: a two-triangle
// emitter, a five-triangle emitter, two strands, two environments, three textures. Expectations are written out by hand or, where the
// arithmetic is shared with the device (unit/object_math.h, unit/light_math.h), formed with those functions called directly.
#include <cstdio>
#include <cstring>
#include <vector>

#include "upload_stages.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) printf("FAILED line %d: %s\n", __LINE__, #cond), failures++; \
  } while (0)

static bool same(const yhd_float4& a, float x, float y, float z, float w) { return a.x == x && a.y == y && a.z == z && a.w == w; }

namespace {
struct Scene {
  // shape 0: a 2 x 1 rectangle of two triangles (area 1 each); shape 1: a fan of five triangles with legs that are no binary fractions;
  // shape 2: two strands of two segments
  std::vector<float> pos0 = {0, 0, 0, 2, 0, 0, 2, 1, 0, 0, 1, 0};
  std::vector<int>   tri0 = {0, 1, 2, 0, 2, 3};
  std::vector<float> pos1 = {0, 0, 0, 0.1f, 0, 0, 0.1f, 0.3f, 0, 0, 0.7f, 0, -0.9f, 0.7f, 0, -1.1f, 0, 0.3f, 0, -1.3f, 0.1f};
  std::vector<int>   tri1 = {0, 1, 2, 0, 2, 3, 0, 3, 4, 0, 4, 5, 0, 5, 6};
  std::vector<float> pos2 = {0, 0, 0, 0, 1, 0, 0, 2, 0, 1, 0, 0, 1, 1, 0, 1, 2, 0};
  std::vector<int>   lin2 = {0, 1, 1, 2, 3, 4, 4, 5};
  yh_shape           shapes[3];
  yh_material        materials[2];
  yh_material_maps   maps[2];
  yh_object          objects[3];
  yh_environment     envs[2];
  std::vector<float> env_texels = {1, 0, 0, 0, 2, 0, 0, 0, 3, 0.5f, 0.25f, 4};  // 2 x 2
  unsigned char      tex_b2[6] = {255, 0, 128, 10, 11, 12};                     // byte, 2 x 1
  float              tex_f2[6] = {0.5f, 1.5f, -1, 7, 8, 9};                     // float, 1 x 2
  unsigned char      tex_b1[3] = {1, 2, 3};                                     // byte, 1 x 1
  yh_texture         textures[3];
  yh_scene_desc      sd;
  Scene() {
    memset(shapes, 0, sizeof(shapes)), memset(materials, 0, sizeof(materials)), memset(maps, 0, sizeof(maps));
    memset(objects, 0, sizeof(objects)), memset(envs, 0, sizeof(envs)), memset(&sd, 0, sizeof(sd)), memset(textures, 0, sizeof(textures));
    shapes[0].num_vertices = 4, shapes[0].positions = pos0.data(), shapes[0].num_triangles = 2, shapes[0].triangles = tri0.data();
    shapes[1].num_vertices = 7, shapes[1].positions = pos1.data(), shapes[1].num_triangles = 5, shapes[1].triangles = tri1.data();
    shapes[2].num_vertices = 6, shapes[2].positions = pos2.data(), shapes[2].num_lines = 4, shapes[2].lines = lin2.data();
    materials[1].emission[0] = 3;
    const float frame[12] = {2, 0, 0, 0, 3, 0, 0, 0, 4, 1, 2, 3};  // not rigid: the object rows invert it in full
    for (int i = 0; i < 3; i++) memcpy(objects[i].frame, frame, 48), objects[i].shape = i, objects[i].material = i < 2 ? 1 : 0;
    const float rigid[12] = {0, 1, 0, -1, 0, 0, 0, 0, 1, 5, 6, 7};
    for (int i = 0; i < 2; i++) memcpy(envs[i].frame, rigid, 48), envs[i].emission[1] = 1.0f + i;
    envs[1].tex_width = 2, envs[1].tex_height = 2, envs[1].texels = env_texels.data();
    textures[0] = {2, 1, 1, tex_b2}, textures[1] = {1, 2, 0, tex_f2}, textures[2] = {1, 1, 1, tex_b1};
    sd.num_shapes = 3, sd.shapes = shapes, sd.num_materials = 2, sd.materials = materials, sd.num_objects = 3, sd.objects = objects;
    sd.num_environments = 2, sd.environments = envs, sd.num_textures = 3, sd.textures = textures;
  }
};
}  // namespace

static void test_object_row() {
  Scene             s;
  const ObjectShape shape{YH_KIND_TRIANGLES, 120, 7, 9, 1, 0, 4000, {5000, 6000, 7000}};
  const yhh::Box    box{{-1, -2, -3}, {1, 4, 9}};
  yhd_object        d;
  memset(&d, 0xff, sizeof(d));
  s.objects[1].material = 1;
  object_row(s.objects[1], shape, box, d);
  float inv[12], lo[4], hi[4];
  inverse_frame(s.objects[1].frame, true, inv);
  padded_world_box(box.min, box.max, lo, hi);
  CHECK(memcmp(d.frame, s.objects[1].frame, 48) == 0 && memcmp(d.inv_frame, inv, 48) == 0);
  CHECK(inv[0] == 0.5f && inv[4] == 1 / 3.0f * 1 && inv[8] == 0.25f);  // (the frame scales by 2, 3, 4)
  CHECK(d.kind == YH_KIND_TRIANGLES && d.node_base == 0 && d.prim_base == 120 && d.vert_base == 7 && d.elem_base == 9);
  CHECK(d.has_normals == 1 && d.material == 1 && d.has_texcoords == 0);
  CHECK(d.lane_root == 5000 && d.lane_test == 4000 && d.lane_root8 == 6000 && d.lane_root16 == 7000);
  CHECK(memcmp(d.wbox_min, lo, 16) == 0 && memcmp(d.wbox_max, hi, 16) == 0);
  CHECK(d.wbox_min[0] < -1 && d.wbox_max[2] > 9 && d.wbox_min[3] == 0 && d.wbox_max[3] == 0);  // (the margin: 1e-3 x the extent 12 + 1e-5)
}

static void test_lights() {
  Scene           s;
  yhd_environment rows[YH_MAX_ENVS];
  memset(rows, 0, sizeof(rows));
  std::vector<yhd_float4> env_texels;
  float emission[3 * YH_MAX_ENVS] = {};
  int   texel_count[YH_MAX_ENVS]  = {};
  environment_rows(s.sd, rows, env_texels, emission, texel_count);
  float inv[12];
  inverse_frame(s.envs[0].frame, false, inv);
  CHECK(memcmp(rows[1].inv_frame, inv, 48) == 0 && memcmp(rows[1].frame, s.envs[1].frame, 48) == 0);
  CHECK(rows[0].tex_w == 0 && rows[0].tex_h == 0 && rows[0].texel_base == 0 && rows[1].tex_w == 2 && rows[1].tex_h == 2 && rows[1].texel_base == 0);
  CHECK(env_texels.size() == 4 && same(env_texels[1], 0, 2, 0, 0) && same(env_texels[3], 0.5f, 0.25f, 4, 0));
  CHECK(emission[1] == 1 && emission[4] == 2 && texel_count[0] == 0 && texel_count[1] == 4);

  const LightShape shapes[3] = {{false, 2}, {false, 5}, {true, 4}};
  LightLayout      L;
  int              at = -1;
  CHECK(light_layout({3, s.objects, s.materials, shapes, 2, emission, texel_count}, L, &at) == YH_LIGHTS_OK);
  CHECK(L.num_lights == 4 && L.cdf_total == 2 + 5 + 4);  // the two emitters, the constant environment (no cdf), the textured one
  std::vector<float> cdf;
  light_cdfs(s.sd, L, cdf);
  CHECK(cdf.size() == L.cdf_total);
  CHECK(cdf[0] == 1 && cdf[1] == 2);  // two triangles of area 1
  {  // the fan: one float chain in element order, every entry the rounded sum of the entry before it and the triangle's area
    float chain = 0;
    bool  rounds = false;
    for (int t = 0; t < 5; t++) {
      const int*  v    = &s.tri1[3 * (size_t)t];
      const float area = triangle_area(ld3(&s.pos1[3 * (size_t)v[0]]), ld3(&s.pos1[3 * (size_t)v[1]]), ld3(&s.pos1[3 * (size_t)v[2]]));
      rounds = rounds || (double)chain + (double)area != (double)(float)(chain + area);
      chain  = t ? chain + area : area;
      CHECK(cdf[2 + (size_t)t] == chain);
    }
    CHECK(rounds);  // (the case can tell a float chain from a sum kept in double)
  }
  {  // the texel cdf: max(rgb) x sin of the row's polar angle, chained
    const float pi = (float)3.14159265358979323846, mx[4] = {1, 2, 3, 4};
    float       chain = 0;
    for (int i = 0; i < 4; i++) {
      const float value = mx[i] * std::sin((i / 2 + 0.5f) * pi / 2);
      chain = i ? value + chain : value;
      CHECK(cdf[7 + (size_t)i] == chain);
    }
  }
  // ---- the record of the small light (object 0): root box with the count in b0.w, the total in b1.w, the triangles' first three
  // float4 each, zeros up to YH_SMALL_LIGHT_TRIS triangles, the cdf row ----
  static_assert(YH_SMALL_LIGHT_TRIS == 4 && YH_SMALL_LIGHT_F4 == 15, "the figures below are written for these");
  CHECK(L.lights[0].small_base == 0 && L.lights[1].small_base == -1);
  std::vector<yhd_float4> rec(12);
  for (int k = 0; k < 12; k++) rec[(size_t)k] = {(float)k, k + 0.25f, k + 0.5f, k + 0.75f};
  const yhh::Box          root{{0, 0, 0}, {2, 1, 0}};
  std::vector<yhd_float4> table;
  small_light_record(L.lights[0], root, rec.data(), cdf.data(), table);
  CHECK(table.size() == 15);
  int count_bits = 0;
  memcpy(&count_bits, &table[0].w, 4);
  CHECK(table[0].x == 0 && table[0].y == 0 && table[0].z == 0 && count_bits == 2);
  CHECK(same(table[1], 2, 1, 0, 2.0f));
  for (int k = 0; k < 3; k++) CHECK(memcmp(&table[2 + (size_t)k], &rec[(size_t)k], 16) == 0 && memcmp(&table[5 + (size_t)k], &rec[6 + (size_t)k], 16) == 0);
  for (int k = 8; k < 14; k++) CHECK(same(table[(size_t)k], 0, 0, 0, 0));
  CHECK(same(table[14], 1, 2, 0, 0));
}

static void test_coarse_index() {
  for (int n : {4096, 4097}) {
    yh_material black;
    memset(&black, 0, sizeof(black));
    const float emission[3] = {0, 1, 0};
    LightLayout L;
    int         at = -1;
    CHECK(light_layout({0, nullptr, &black, nullptr, 1, emission, &n}, L, &at) == YH_LIGHTS_OK && L.env_tab_light == 0);
    std::vector<float> cdf((size_t)n), tab;
    for (int i = 0; i < n; i++) cdf[(size_t)i] = (float)(i + 1);  // (entry i holds i + 1: an index entry names the entry it copies)
    coarse_index(L, cdf.data(), tab);
    if (n == 4096) {  // every 2nd entry, 2048 of them
      CHECK(tab.size() == 2048 && tab[0] == 2 && tab[1] == 4 && tab[2047] == 4096);
    } else {  // every 3rd, 1366 of them; the last one is the cdf's last entry
      CHECK(tab.size() == 1366 && tab[0] == 3 && tab[1] == 6 && tab[1364] == 4095 && tab[1365] == 4097);
    }
  }
  LightLayout none;
  std::vector<float> tab;
  coarse_index(none, nullptr, tab);
  CHECK(tab.empty());
}

static float srgb_to_rgb(float srgb) { return (srgb <= 0.04045) ? srgb / 12.92f : std::pow((srgb + 0.055f) / (1.0f + 0.055f), 2.4f); }

static void test_textures() {
  std::vector<yhd_texture> tex;
  std::vector<yhd_float4>  texels;
  int                      at = -1;
  {  // maps in force: texture 1 (bytes) is a colour texture and a roughness map, 2 (floats) a scattering texture, 3 only a transmission map
    Scene s;
    s.materials[0].color_tex = 1, s.maps[0].roughness_tex = 1;
    s.materials[1].scattering_tex = 2, s.maps[1].transmission_tex = 3;
    CHECK(convert_textures(s.sd, s.maps, tex, texels, &at) == YH_TEXTURES_OK);
    CHECK(tex.size() == 3 && texels.size() == 6);
    CHECK(tex[0].width == 2 && tex[0].height == 1 && tex[0].srgb_base == 0 && tex[0].linear_base == 2);  // the linear copy behind the decoded one
    CHECK(tex[1].width == 1 && tex[1].height == 2 && tex[1].srgb_base == 4 && tex[1].linear_base == 4);  // floats: one copy
    CHECK(tex[2].width == 1 && tex[2].height == 1 && tex[2].srgb_base == -1 && tex[2].linear_base == -1);  // not uploaded
    CHECK(same(texels[0], 1, 0, srgb_to_rgb(128 / 255.0f), 0) && same(texels[1], srgb_to_rgb(10 / 255.0f), srgb_to_rgb(11 / 255.0f), srgb_to_rgb(12 / 255.0f), 0));
    CHECK(texels[1].x == (10 / 255.0f) / 12.92f && texels[0].z > 0.2f && texels[0].z < 0.22f);  // (below the knee: linear; 128: 0.2158...)
    CHECK(same(texels[2], 1, 0, 128 / 255.0f, 0) && same(texels[3], 10 / 255.0f, 11 / 255.0f, 12 / 255.0f, 0));
    CHECK(same(texels[4], 0.5f, 1.5f, -1, 0) && same(texels[5], 7, 8, 9, 0));
  }
  {  // no maps in force: every texture is uploaded; a linear copy only of what an emission texture names
    Scene s;
    s.materials[0].color_tex = 1, s.materials[1].emission_tex = 3;
    texels.clear();
    CHECK(convert_textures(s.sd, nullptr, tex, texels, &at) == YH_TEXTURES_OK);
    CHECK(texels.size() == 2 + 2 + 1 + 1);
    CHECK(tex[0].srgb_base == 0 && tex[0].linear_base == -1 && tex[1].srgb_base == 2 && tex[1].linear_base == 2 && tex[2].srgb_base == 4 && tex[2].linear_base == 5);
    CHECK(same(texels[5], 1 / 255.0f, 2 / 255.0f, 3 / 255.0f, 0));
  }
  {  // an empty texture, an id one past the end: their codes, with the texture and the material
    Scene s;
    s.textures[1].width = 0;
    texels.clear(), at = -1;
    CHECK(convert_textures(s.sd, nullptr, tex, texels, &at) == YH_TEXTURES_EMPTY && at == 1);
    s.textures[1].width = 1, s.textures[2].pixels = nullptr, at = -1;
    texels.clear();
    CHECK(convert_textures(s.sd, nullptr, tex, texels, &at) == YH_TEXTURES_EMPTY && at == 2);
    Scene t;
    t.materials[1].color_tex = 4, at = -1;
    texels.clear();
    CHECK(convert_textures(t.sd, nullptr, tex, texels, &at) == YH_TEXTURES_MISSING && at == 1);
    t.materials[1].color_tex = 3, t.materials[0].scattering_tex = -1, at = -1;
    CHECK(convert_textures(t.sd, nullptr, tex, texels, &at) == YH_TEXTURES_MISSING && at == 0);
    t.materials[0].scattering_tex = 3;
    CHECK(convert_textures(t.sd, nullptr, tex, texels, &at) == YH_TEXTURES_OK);
  }
}

static void test_key_bytes() {
  Scene                      s;
  std::vector<float>         many(3 * 600);
  for (size_t i = 0; i < many.size(); i++) many[i] = (float)i;
  s.shapes[2].num_vertices = 600, s.shapes[2].positions = many.data();  // more than 2 x 256 vertices: the first and the last 256 only
  std::vector<unsigned char> geometry = {9, 9}, envs = {9};
  std::vector<size_t>        key_positions;
  description_key_bytes(s.sd, geometry, envs, key_positions);
  const size_t rows = 3 * sizeof(yh_object);
  CHECK(key_positions.size() == 3 && key_positions[0] == rows + 12 && key_positions[1] == rows + 12 + 2 * 4 * 12 + 12);
  CHECK(key_positions[2] == key_positions[1] + 2 * 7 * 12 + 12 && geometry.size() == key_positions[2] + 2 * 256 * 12);
  CHECK(memcmp(geometry.data(), s.objects, rows) == 0);
  const int counts0[3] = {4, 0, 2}, counts2[3] = {600, 4, 0};
  CHECK(memcmp(geometry.data() + rows, counts0, 12) == 0 && memcmp(geometry.data() + key_positions[2] - 12, counts2, 12) == 0);
  CHECK(memcmp(geometry.data() + key_positions[0], s.pos0.data(), 48) == 0 && memcmp(geometry.data() + key_positions[0] + 48, s.pos0.data(), 48) == 0);  // (4 vertices: both samples are all of them)
  CHECK(memcmp(geometry.data() + key_positions[2], many.data(), 256 * 12) == 0 && memcmp(geometry.data() + key_positions[2] + 256 * 12, many.data() + 3 * (600 - 256), 256 * 12) == 0);
  const size_t head = offsetof(yh_environment, texels);
  CHECK(envs.size() == 2 * head && memcmp(envs.data(), &s.envs[0], head) == 0 && memcmp(envs.data() + head, &s.envs[1], head) == 0);
}

int main() {
  test_object_row();
  test_lights();
  test_coarse_index();
  test_textures();
  test_key_bytes();
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("all checks passed\n");
  return 0;
}
