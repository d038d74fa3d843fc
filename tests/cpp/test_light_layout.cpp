// The rule that makes the light list (yocto-hair_amd/host/light_layout.h), without a device: which objects and environments are lights,
// in which order, and where their entries sit. Every expectation below is written out by hand from the rule (include/yhair.h: "THE LIGHT
// LIST", csrc/yh_device.h: yhd_light), none is computed by the function under test.
#include <cstdio>
#include <cstring>
#include <vector>

#include "light_layout.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) printf("FAILED line %d: %s\n", __LINE__, #cond), failures++; \
  } while (0)

// a scene description in the function's terms. Materials: 0 black, 1 emits. Shapes are given per case.
namespace {
struct Scene {
  std::vector<yh_object>   objects;
  std::vector<yh_material> materials;
  std::vector<LightShape>  shapes;
  std::vector<float>       emission;  // 3 per environment
  std::vector<int>         texels;
  Scene() {
    materials.resize(2);
    memset(materials.data(), 0, sizeof(yh_material) * 2);
    materials[1].emission[1] = 2.0f;  // (one non-zero channel is enough)
  }
  void object(int shape, int material) {
    yh_object o;
    memset(&o, 0, sizeof(o));
    o.shape = shape, o.material = material;
    objects.push_back(o);
  }
  void environment(bool emits, int texel_count) {
    emission.push_back(0), emission.push_back(0), emission.push_back(emits ? 0.5f : 0.0f);
    texels.push_back(texel_count);
  }
  int layout(LightLayout& out, int* at) const {
    const LightLayoutIn in{(int)objects.size(), objects.data(), materials.data(), shapes.data(), (int)texels.size(), emission.data(), texels.data()};
    return light_layout(in, out, at);
  }
};
}  // namespace

static bool row_is(const yhd_light& l, int object, int environment, int cdf_base, int cdf_count, int small_base) {
  return l.object == object && l.environment == environment && l.cdf_base == cdf_base && l.cdf_count == cdf_count && l.small_base == small_base;
}

int main() {
  static_assert(YH_MAX_LIGHTS == 16 && YH_SMALL_LIGHT_TRIS == 4 && YH_SMALL_LIGHT_F4 == 15, "the figures below are written for these");
  LightLayout L;
  int         at = -1;
  {  // (a) objects and environments "interleaved": the description lists environments and objects apart, the emitters among each are
     // scattered between non-emitters. Objects first, in order, then environments, in order; cdf_base runs through both groups.
    Scene s;
    s.shapes = {{false, 10}, {false, 7}};
    s.environment(true, 100);   // environment 0: 10 x 10 texels
    s.object(0, 0);             // object 0: black
    s.object(1, 1);             // object 1: emits, 7 triangles
    s.environment(false, 64);   // environment 1: black
    s.object(0, 1);             // object 2: emits, 10 triangles
    s.object(1, 0);             // object 3: black
    s.environment(true, 36);    // environment 2
    CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 4);
    CHECK(row_is(L.lights[0], 1, -1, 0, 7, -1));
    CHECK(row_is(L.lights[1], 2, -1, 7, 10, -1));
    CHECK(row_is(L.lights[2], -1, 0, 17, 100, -1));
    CHECK(row_is(L.lights[3], -1, 2, 117, 36, -1));
    CHECK(L.cdf_total == 153 && L.big_lights && L.table_f4 == 0);
    CHECK(L.env_tab_light == -1 && L.env_tab_k == 0 && L.env_tab_stride == 0);
  }
  {  // (b) an emissive material on a line shape and on a shape of 0 triangles: neither is a light
    Scene s;
    s.shapes = {{true, 500}, {false, 0}, {false, 2}};
    s.object(0, 1), s.object(1, 1), s.object(2, 1);
    CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 1 && row_is(L.lights[0], 2, -1, 0, 2, 0));
    CHECK(L.cdf_total == 2 && !L.big_lights && L.table_f4 == 15);
    Scene none;  // ... and on their own they leave the scene without a light
    none.shapes = {{true, 500}, {false, 0}};
    none.object(0, 1), none.object(1, 1);
    CHECK(none.layout(L, &at) == YH_LIGHTS_NONE);
  }
  {  // (c) emitters of 4 and 5 triangles: the first has its record in the LDS table, the second is read through memory
    Scene s;
    s.shapes = {{false, 4}, {false, 5}};
    s.object(0, 1), s.object(1, 1), s.object(0, 1);
    CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 3);
    CHECK(row_is(L.lights[0], 0, -1, 0, 4, 0));
    CHECK(row_is(L.lights[1], 1, -1, 4, 5, -1));
    CHECK(row_is(L.lights[2], 2, -1, 9, 4, 15));  // (the second small record follows the first)
    CHECK(L.table_f4 == 30 && L.big_lights && L.cdf_total == 13);
    Scene small;
    small.shapes = {{false, 4}};
    small.object(0, 1);
    CHECK(small.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 1 && row_is(L.lights[0], 0, -1, 0, 4, 0) && L.table_f4 == 15 && !L.big_lights);
  }
  {  // (d) 16 lights pass; a 17th as an object and as an environment: each its own code, with the index of the one too many
    Scene s;
    s.shapes = {{false, 1}};
    s.object(0, 0);  // object 0: black
    for (int i = 0; i < 15; i++) s.object(0, 1);  // objects 1 .. 15: lights 0 .. 14
    s.environment(false, 0);
    s.environment(true, 0);  // environment 1: light 15
    CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 16 && row_is(L.lights[14], 15, -1, 14, 1, 14 * 15) && row_is(L.lights[15], -1, 1, 15, 0, -1));
    CHECK(L.table_f4 == 15 * 15 && L.cdf_total == 15);
    Scene env17 = s;
    env17.environment(false, 0);
    env17.environment(true, 0);  // environment 3: the 17th
    at = -1;
    CHECK(env17.layout(L, &at) == YH_LIGHTS_ENVIRONMENT_TOO_MANY && at == 3);
    Scene obj17;
    obj17.shapes = {{false, 1}};
    obj17.object(0, 0), obj17.object(0, 0);  // objects 0, 1: black
    for (int i = 0; i < 16; i++) obj17.object(0, 1);  // objects 2 .. 17: lights 0 .. 15
    obj17.object(0, 0);                                // object 18: black
    obj17.object(0, 1);                                // object 19: the 17th
    at = -1;
    CHECK(obj17.layout(L, &at) == YH_LIGHTS_OBJECT_TOO_MANY && at == 19);
    obj17.objects.pop_back();
    CHECK(obj17.layout(L, &at) == YH_LIGHTS_OK && L.num_lights == 16 && L.lights[15].object == 17);
  }
  {  // (e) no emitter at all
    Scene s;
    s.shapes = {{false, 12}};
    s.object(0, 0);
    s.environment(false, 4096);
    CHECK(s.layout(L, &at) == YH_LIGHTS_NONE);
    Scene empty;
    CHECK(empty.layout(L, &at) == YH_LIGHTS_NONE);
  }
  {  // (f) the coarse index of a texel cdf: from 4096 texels on; stride = ceil(n / 2048), k = ceil(n / stride)
    struct { int n, light, k, stride; } cases[] = {
        {4095, -1, 0, 0},
        {4096, 0, 2048, 2},          // stride (4096 + 2047) / 2048 = 2, k = 4096 / 2
        {4097, 0, 1366, 3},          // stride (4097 + 2047) / 2048 = 3, k = ceil(4097 / 3) = 1366 (3 * 1365 = 4095)
        {2048 * 3 + 1, 0, 1537, 4},  // 6145: stride (6145 + 2047) / 2048 = 4, k = ceil(6145 / 4) = 1537 (4 * 1536 = 6144)
    };
    for (auto& c : cases) {
      Scene s;
      s.environment(true, c.n);
      CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
      CHECK(L.num_lights == 1 && row_is(L.lights[0], -1, 0, 0, c.n, -1) && L.cdf_total == (size_t)c.n);
      CHECK(L.env_tab_light == c.light && L.env_tab_k == c.k && L.env_tab_stride == c.stride);
    }
    Scene two;  // two qualify: only the FIRST gets the index; a smaller one in front of them gets none
    two.shapes = {{false, 3}};
    two.object(0, 1);            // light 0
    two.environment(true, 4095); // light 1: too small
    two.environment(true, 6145); // light 2: the index
    two.environment(true, 4096); // light 3: qualifies, but is not the first
    CHECK(two.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 4 && L.env_tab_light == 2 && L.env_tab_k == 1537 && L.env_tab_stride == 4);
    CHECK(row_is(L.lights[2], -1, 1, 3 + 4095, 6145, -1) && row_is(L.lights[3], -1, 2, 3 + 4095 + 6145, 4096, -1));
    Scene area;  // an AREA light of 4096 triangles gets no index: it is the texel cdf's
    area.shapes = {{false, 4096}};
    area.object(0, 1);
    CHECK(area.layout(L, &at) == YH_LIGHTS_OK && L.env_tab_light == -1);
  }
  {  // (g) a constant environment: no cdf, and the next light's segment begins where its own would have
    Scene s;
    s.environment(true, 0);
    s.environment(true, 9);
    CHECK(s.layout(L, &at) == YH_LIGHTS_OK);
    CHECK(L.num_lights == 2 && row_is(L.lights[0], -1, 0, 0, 0, -1) && row_is(L.lights[1], -1, 1, 0, 9, -1));
    CHECK(L.cdf_total == 9 && !L.big_lights && L.table_f4 == 0 && L.env_tab_light == -1);
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("all checks passed\n");
  return 0;
}
