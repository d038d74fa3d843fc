// tests/test_light_edits.py: with the mirror's opt-in (set_light_edits, an extension) what changes the LIGHT LIST — an emission turned on
// or off, set_material that makes an object a light or takes that away (under set_object_edits), a vertex edit of an emitter's shape
// (under set_shape_edits) — goes through the yh_update_* calls at the next init_state (scene::edits counts) and not through the whole
// upload (scene::uploads); without the opt-in the mirror classifies as before (tests/cpp/test_mirror_edits.cpp pins that).
//   test_mirror_light_edits --classify       the classification alone (detail::classify_edit, a pure function): no device needed
//   test_mirror_light_edits <scene.json>     the classification, then renders of lights-unit on the device: every edited render is
//                                            compared bit for bit with the render of a scene built with the edit from the start
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

namespace yd = yhair::detail;

static void classification() {
  static float positions[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, other_positions[9] = {0, 0, 0, 2, 0, 0, 0, 2, 0};
  static int   triangle[3]  = {0, 1, 2};
  yd::flat_scene base;
  yh_shape       sh{};
  sh.num_vertices = 3, sh.positions = positions, sh.num_triangles = 1, sh.triangles = triangle;
  base.shapes = {sh, sh};
  base.shape_vertex_edits = {0, 0};
  yh_material grey{}, lamp{};
  grey.color[0] = grey.color[1] = grey.color[2] = 0.5f, grey.opacity = 1, grey.ior = 1.5f, grey.trdepth = 0.01f;
  lamp = grey, lamp.emission[0] = lamp.emission[1] = lamp.emission[2] = 5;
  base.materials = {grey, lamp};
  base.maps.assign(2, yh_material_maps{});
  yh_object ob{};
  ob.frame[0] = ob.frame[4] = ob.frame[8] = 1;
  base.objects = {ob, ob};  // shape 0 under the lamp, shape 1 grey
  base.objects[0].material = 1, base.objects[1].shape = 1;
  yh_environment env{};
  env.frame[0] = env.frame[4] = env.frame[8] = 1, env.emission[0] = env.emission[1] = env.emission[2] = 0.5f;
  base.environments = {env};
  base.camera.frame[0] = base.camera.frame[4] = base.camera.frame[8] = 1, base.camera.lens = 0.05f, base.camera.film[0] = 0.036f, base.camera.film[1] = 0.024f;
  base.camera.focus = 10000;

  // an emission toggle of a material, on and off: the upload as today, an edit with the opt-in
  auto now = base;
  now.materials[0].emission[1] = 1;
  CHECK(yd::classify_edit(base, now) == yd::edit_upload && yd::classify_edit(base, now, true, true) == yd::edit_upload);
  CHECK(yd::classify_edit(base, now, false, false, true) == yd::edit_materials);
  now = base, now.materials[1].emission[0] = now.materials[1].emission[1] = now.materials[1].emission[2] = 0;
  CHECK(yd::classify_edit(base, now) == yd::edit_upload && yd::classify_edit(base, now, false, false, true) == yd::edit_materials);
  // ... of an environment
  now = base, now.environments[0].emission[0] = now.environments[0].emission[1] = now.environments[0].emission[2] = 0;
  CHECK(yd::classify_edit(base, now) == yd::edit_upload && yd::classify_edit(base, now, false, false, true) == yd::edit_environments);
  // an object that takes the lamp: needs the object opt-in too
  now = base, now.objects[1].material = 1;
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload && yd::classify_edit(base, now, false, false, true) == yd::edit_upload);
  CHECK(yd::classify_edit(base, now, true, false, true) == yd::edit_objects);
  // the vertices of the emitter's shape: needs the shape opt-in too
  now = base, now.shapes[0].positions = other_positions;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload && yd::classify_edit(base, now, false, false, true) == yd::edit_upload);
  CHECK(yd::classify_edit(base, now, false, true, true) == yd::edit_shapes);
  // what stays an upload with every opt-in: a texture id, a count, an environment's texture
  now = base, now.materials[1].emission_tex = 1;
  CHECK(yd::classify_edit(base, now, true, true, true) == yd::edit_upload);
  now = base, now.shapes[0].num_triangles = 0;
  CHECK(yd::classify_edit(base, now, true, true, true) == yd::edit_upload);
  now = base, now.environments[0].tex_width = 2;
  CHECK(yd::classify_edit(base, now, true, true, true) == yd::edit_upload);
  // ... and nothing else changes its class
  now = base, now.camera.focus = 3, now.materials[0].color[1] = 0.1f;
  CHECK(yd::classify_edit(base, now, false, false, true) == (yd::edit_camera | yd::edit_materials) && yd::classify_edit(base, base, true, true, true) == yd::edit_none);
}

struct Built {
  std::unique_ptr<ptr::scene> scene = std::make_unique<ptr::scene>();
  ptr::camera*                camera = nullptr;
  std::vector<ptr::object*>   lamps;  // the objects whose material emits, in scene order
  ptr::material*              dark = nullptr;
};
static Built build(const yh_scene_file* file, const ptr::trace_params& params, bool opt_in) {
  Built b;
  b.camera = init_scene(b.scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
  for (auto& o : b.scene->objects) {
    const auto& e = o->material_->emission;
    if (e.x != 0 || e.y != 0 || e.z != 0) b.lamps.push_back(o.get());
    else if (!b.dark) b.dark = o->material_;
  }
  ptr::set_light_edits(b.scene.get(), opt_in), ptr::set_object_edits(b.scene.get(), opt_in), ptr::set_shape_edits(b.scene.get(), opt_in);
  ptr::init_bvh(b.scene.get(), params);
  ptr::init_lights(b.scene.get(), params);
  return b;
}
static std::vector<vec4f> render(Built& b, const ptr::trace_params& params) {
  ptr::state st;
  ptr::init_state(&st, b.scene.get(), b.camera, params);
  ptr::trace_samples(&st, b.scene.get(), b.camera, params, params.samples);
  return st.render;
}
static bool same(const std::vector<vec4f>& a, const std::vector<vec4f>& b) {
  return a.size() == b.size() && !a.empty() && !memcmp(a.data(), b.data(), a.size() * sizeof(vec4f));
}
// the three edits, in the order the test makes them
static void mute(Built& b) { ptr::set_emission(b.lamps[0]->material_, {0, 0, 0}); }
static void sky_off(Built& b) { ptr::set_emission(b.scene->environments[0].get(), {0, 0, 0}, b.scene->environments[0]->emission_tex); }
static void darken(Built& b) { ptr::set_material(b.lamps[1], b.dark); }
static void relight(Built& b) { ptr::set_emission(b.lamps[0]->material_, {4, 5, 6}); }
static void stretch(Built& b) {
  auto positions = b.lamps[0]->shape_->positions;  // (a copy of the same size: the setter writes into the shape's own storage)
  for (auto& p : positions) p.x = 1.5f * p.x + 0.25f * p.y, p.y *= 0.75f;
  ptr::set_positions(b.lamps[0]->shape_, positions);
}

int main(int argc, const char* argv[]) {
  if (argc < 2) return 2;
  classification();
  if (failures) return 10;
  if (!strcmp(argv[1], "--classify")) {
    printf("ok\n");
    return 0;
  }
  try {
    char err[512] = "";
    auto file     = yh_scene_load(argv[1], "", err, sizeof(err));
    if (!file) print_fatal(err);
    auto params       = ptr::trace_params{};
    params.resolution = 48, params.samples = 2;

    Built a    = build(file, params, true);
    auto  img0 = render(a, params);
    CHECK(a.lamps.size() == 2 && a.dark != nullptr && a.scene->environments.size() == 1);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 0);
    mute(a);
    auto img_mute = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1 && !same(img_mute, img0));
    sky_off(a);
    auto img_sky = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 2 && !same(img_sky, img_mute));
    relight(a), darken(a);
    auto img_dark = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 3 && !same(img_dark, img_sky));
    stretch(a);
    auto img_stretch = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 4 && !same(img_stretch, img_dark));
    // the only light left turned off: the contexts refuse, the mirror falls back to the upload, which says why
    mute(a);
    bool threw = false;
    try {
      render(a, params);
    } catch (const std::exception& e) {
      threw = strstr(e.what(), "no lights") != nullptr;
    }
    CHECK(threw && a.scene->edits == 4);

    // the same scenes, each built with its edits from the start; without the opt-in a toggle is the upload, as before
    Built b = build(file, params, false);
    mute(b);
    CHECK(same(render(b, params), img_mute) && b.scene->uploads == 1 && b.scene->edits == 0);
    sky_off(b);
    CHECK(same(render(b, params), img_sky) && b.scene->uploads == 2 && b.scene->edits == 0);
    relight(b), darken(b);
    CHECK(same(render(b, params), img_dark) && b.scene->uploads == 3);
    stretch(b);
    ptr::init_bvh(b.scene.get(), params);  // (without set_shape_edits a setter that writes into the shape's own storage is not seen: the way to force the upload)
    CHECK(same(render(b, params), img_stretch) && b.scene->uploads == 4 && b.scene->edits == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
