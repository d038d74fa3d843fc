// tests/test_object_edits.py: with the mirror's opt-in (set_object_edits, an extension) an object's frame or material set after an
// init_state goes through yh_update_objects at the next one (scene::edits counts) and not through the whole upload (scene::uploads);
// without the opt-in the mirror classifies and behaves as before (tests/cpp/test_mirror_edits.cpp pins that).
//   test_mirror_object_edits --classify       the classification alone (detail::classify_edit, a pure function): no device needed
//   test_mirror_object_edits <scene.json>     the classification, then renders on the device: set_frame on the hair object with the
//                                             opt-in is one edit, and its pixels are those of a scene built that way from the start
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

namespace yd = yhair::detail;

static void classification() {
  static float         positions[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, other_positions[9] = {0, 0, 0, 2, 0, 0, 0, 2, 0};
  static int           triangle[3]  = {0, 1, 2};
  static unsigned char pixels[3] = {1, 2, 3}, other_pixels[3] = {4, 5, 6};
  yd::flat_scene base;
  yh_shape       sh{};
  sh.num_vertices = 3, sh.positions = positions, sh.num_triangles = 1, sh.triangles = triangle;
  base.shapes = {sh, sh};
  base.shapes[1].positions = other_positions;
  yh_material grey{}, lamp{}, blue{};
  grey.color[0] = grey.color[1] = grey.color[2] = 0.5f, grey.opacity = 1, grey.ior = 1.5f, grey.trdepth = 0.01f;
  lamp = grey, lamp.emission[0] = lamp.emission[1] = lamp.emission[2] = 5;
  blue = grey, blue.color[2] = 0.9f;
  base.materials = {grey, lamp, blue};
  base.maps.assign(3, yh_material_maps{});
  yh_object ob{};
  ob.frame[0] = ob.frame[4] = ob.frame[8] = 1, ob.shape = 0, ob.material = 1;
  base.objects = {ob, ob};
  base.objects[1].material = 0, base.objects[1].frame[9] = 2;
  yh_texture tex{};
  tex.width = tex.height = 1, tex.is_byte = 1, tex.pixels = pixels;
  base.textures = {tex};
  yh_environment env{};
  env.frame[0] = env.frame[4] = env.frame[8] = 1, env.emission[0] = env.emission[1] = env.emission[2] = 0.5f;
  base.environments = {env};
  base.camera.frame[0] = base.camera.frame[4] = base.camera.frame[8] = 1, base.camera.lens = 0.05f, base.camera.film[0] = 0.036f, base.camera.film[1] = 0.024f;
  base.camera.focus = 10000;

  CHECK(yd::classify_edit(base, base, true) == yd::edit_none);
  // with the opt-in: a frame, a material, both, and next to the edits the other calls take
  auto now = base;
  now.objects[1].frame[10] = 0.25f;
  CHECK(yd::classify_edit(base, now, true) == yd::edit_objects);
  now = base, now.objects[1].material = 2;
  CHECK(yd::classify_edit(base, now, true) == yd::edit_objects);
  now = base, now.objects[0].frame[0] = 2, now.objects[1].material = 2, now.objects[1].frame[9] = -1;
  CHECK(yd::classify_edit(base, now, true) == yd::edit_objects);
  now.camera.focus = 3, now.materials[0].beta_m = 0.6f;
  CHECK(yd::classify_edit(base, now, true) == (yd::edit_objects | yd::edit_camera | yd::edit_materials));
  // ... and what yh_update_objects does not take
  now = base, now.objects[1].shape = 1;  // a shape change
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects.push_back(ob);  // an added object
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects.pop_back();
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects[1].frame[10] = 0.25f, now.textures[0].pixels = other_pixels;  // an object change next to a texture change
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects[1].material = 1;  // emission on, by reassignment
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects[0].material = 2;  // ... and off
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  now = base, now.objects[1].material = 7;  // a material outside the table
  CHECK(yd::classify_edit(base, now, true) == yd::edit_upload);
  // without the opt-in: as ever, through either overload
  now = base, now.objects[1].frame[10] = 0.25f;
  CHECK(yd::classify_edit(base, now, false) == yd::edit_upload && yd::classify_edit(base, now) == yd::edit_upload);
  now = base, now.objects[1].material = 2;
  CHECK(yd::classify_edit(base, now, false) == yd::edit_upload && yd::classify_edit(base, now) == yd::edit_upload);
  now = base, now.camera.focus = 3;
  CHECK(yd::classify_edit(base, now, false) == yd::edit_camera && yd::classify_edit(base, now) == yd::edit_camera && yd::classify_edit(base, now, true) == yd::edit_camera);
}

struct Built {
  std::unique_ptr<ptr::scene> scene = std::make_unique<ptr::scene>();
  ptr::camera*                camera = nullptr;
  ptr::object*                hair_object = nullptr;
};
static Built build(const yh_scene_file* file, const ptr::trace_params& params, bool opt_in) {
  Built b;
  b.camera = init_scene(b.scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
  for (auto& o : b.scene->objects)
    if (!o->shape_->lines.empty()) b.hair_object = o.get();
  ptr::set_object_edits(b.scene.get(), opt_in);
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
    params.resolution = 64, params.samples = 2;
    auto moved_object = [](frame3f f) { return f.o.x -= 0.3f, f.o.y += 0.2f, f.x.x *= 1.25f, f; };

    Built a    = build(file, params, true);
    auto  img0 = render(a, params);
    CHECK(a.hair_object != nullptr);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 0);
    ptr::set_frame(a.hair_object, moved_object(a.hair_object->frame));
    auto img_object = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1);
    CHECK(!same(img_object, img0));
    auto again = render(a, params);  // nothing changed since: nothing happens
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1 && same(again, img_object));

    // the same scene built with the moved object from the start
    Built b = build(file, params, false);
    ptr::set_frame(b.hair_object, moved_object(b.hair_object->frame));
    CHECK(same(render(b, params), img_object));
    CHECK(b.scene->uploads == 1 && b.scene->edits == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
