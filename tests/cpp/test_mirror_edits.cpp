// tests/test_scene_edits.py: edits made through the C++ mirror's set_* functions after an init_state take effect at the next one, as
// they do in the reference, which reads its scene structs live (apps/ysceneitraces/ysceneitraces.cpp:392-410) — through the
// yh_update_* calls where those accept the edit (scene::edits counts), through the whole upload otherwise (scene::uploads).
//   test_mirror_edits --classify       the classification alone (detail::classify_edit, a pure function): no device needed
//   test_mirror_edits <scene.json>     the classification, then renders on the device; every edited render is compared bit for bit
//                                      with the render of a second scene object built with the edit from the start
// Exit status 0 and "ok" on success; a failed check prints its line. Without a device the render part ends with the library's message.
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
  base.shapes.push_back(sh);
  yh_material grey{}, lamp{};
  grey.color[0] = grey.color[1] = grey.color[2] = 0.5f, grey.opacity = 1, grey.ior = 1.5f, grey.trdepth = 0.01f;
  lamp = grey, lamp.emission[0] = lamp.emission[1] = lamp.emission[2] = 5;
  base.materials = {grey, lamp};
  base.maps.assign(2, yh_material_maps{});
  yh_object ob{};
  ob.frame[0] = ob.frame[4] = ob.frame[8] = 1, ob.shape = 0, ob.material = 1;
  base.objects = {ob, ob};
  base.objects[1].material = 0, base.objects[1].frame[9] = 2;
  yh_environment env{};
  env.frame[0] = env.frame[4] = env.frame[8] = 1, env.emission[0] = env.emission[1] = env.emission[2] = 0.5f;
  base.environments = {env};
  base.camera.frame[0] = base.camera.frame[4] = base.camera.frame[8] = 1, base.camera.lens = 0.05f, base.camera.film[0] = 0.036f, base.camera.film[1] = 0.024f;
  base.camera.focus = 10000;

  CHECK(yd::classify_edit(base, base) == yd::edit_none);
  auto now = base;
  now.camera.frame[9] = 1, now.camera.aperture = 0.1f;
  CHECK(yd::classify_edit(base, now) == yd::edit_camera);  // camera only
  now = base, now.materials[0].beta_m = 0.6f, now.materials[0].color[1] = 0.1f;
  CHECK(yd::classify_edit(base, now) == yd::edit_materials);  // material only
  now.materials[1].emission[0] = 7;  // (an emitter that stays one)
  CHECK(yd::classify_edit(base, now) == yd::edit_materials);
  now = base, now.environments[0].frame[9] = 1, now.environments[0].emission[2] = 2;
  CHECK(yd::classify_edit(base, now) == yd::edit_environments);
  now.camera.lens = 0.1f, now.materials[0].specular = 0.5f;
  CHECK(yd::classify_edit(base, now) == (yd::edit_camera | yd::edit_materials | yd::edit_environments));
  // ... and what no update call accepts
  now = base, now.materials[0].emission[1] = 1;  // an emission toggle, on
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.materials[1].emission[0] = now.materials[1].emission[1] = now.materials[1].emission[2] = 0;  // ... and off
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.environments[0].emission[0] = now.environments[0].emission[1] = now.environments[0].emission[2] = 0;
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.objects[1].frame[10] = 0.25f;  // an object frame
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.objects[1].material = 1;
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.shapes[0].positions = other_positions;  // a shape pointer
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.shapes[0].num_triangles = 0;
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.materials[0].color_tex = 1;  // a texture id
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.maps[0].opacity_tex = 1;
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.materials.push_back(grey), now.maps.push_back(yh_material_maps{});
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
  now = base, now.camera.focus = 3, now.objects[0].frame[9] = 1;  // an accepted edit next to one that is not
  CHECK(yd::classify_edit(base, now) & yd::edit_upload);
}

struct Built {
  std::unique_ptr<ptr::scene> scene = std::make_unique<ptr::scene>();
  ptr::camera*                camera = nullptr;
  ptr::material*              hair   = nullptr;
  ptr::object*                hair_object = nullptr;
};
static Built build(const yh_scene_file* file, const ptr::trace_params& params) {
  Built b;
  b.camera = init_scene(b.scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
  for (auto& o : b.scene->objects)
    if (!o->shape_->lines.empty()) b.hair = o->material_, b.hair_object = o.get();
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
    auto moved_camera = [](frame3f f) { return f.o.x += 0.4f, f.o.y += 0.3f, f.o.z -= 0.5f, f; };
    auto moved_object = [](frame3f f) { return f.o.x -= 0.3f, f.o.y += 0.2f, f; };

    Built a    = build(file, params);
    auto  img0 = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 0);
    auto again = render(a, params);  // nothing changed: nothing happens
    CHECK(a.scene->uploads == 1 && a.scene->edits == 0 && same(again, img0));
    // set_frame on the same camera object
    ptr::set_frame(a.camera, moved_camera(a.camera->frame));
    auto img_camera = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1);
    CHECK(!same(img_camera, img0));
    // a hair setter on a material
    CHECK(a.hair != nullptr);
    ptr::set_beta_m(a.hair, 0.6f), ptr::set_sigma_a(a.hair, {0.3f, 0.6f, 1.2f});
    auto img_hair = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 2);
    CHECK(!same(img_hair, img_camera));
    // set_frame on an object: the whole upload
    ptr::set_frame(a.hair_object, moved_object(a.hair_object->frame));
    auto img_object = render(a, params);
    CHECK(a.scene->uploads == 2 && a.scene->edits == 2);
    CHECK(!same(img_object, img_hair));

    // the same scenes, each built with its edits from the start
    Built b = build(file, params);
    ptr::set_frame(b.camera, moved_camera(b.camera->frame));
    CHECK(same(render(b, params), img_camera));
    CHECK(b.scene->uploads == 1 && b.scene->edits == 0);
    Built c = build(file, params);
    ptr::set_frame(c.camera, moved_camera(c.camera->frame));
    ptr::set_beta_m(c.hair, 0.6f), ptr::set_sigma_a(c.hair, {0.3f, 0.6f, 1.2f});
    CHECK(same(render(c, params), img_hair));
    ptr::set_frame(c.hair_object, moved_object(c.hair_object->frame));
    CHECK(same(render(c, params), img_object));
    CHECK(c.scene->uploads == 2 && c.scene->edits == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
