// tests/test_shape_edits.py: with the mirror's opt-in (set_shape_edits, an extension) a shape's positions, normals, radius or texcoords
// set after an init_state go through yh_update_shape at the next one (scene::edits counts) and not through the whole upload
// (scene::uploads); without the opt-in the mirror classifies and behaves as before (tests/cpp/test_mirror_edits.cpp pins that).
//   test_mirror_shape_edits --classify       the classification alone (detail::classify_edit, a pure function): no device needed
//   test_mirror_shape_edits <scene.json>     the classification, then renders on the device: set_positions / set_normals on the hair with
//                                            the opt-in is one edit, and its pixels are those of a scene built that way from the start
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

namespace yd = yhair::detail;

static void classification() {
  static float positions[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, other_positions[9] = {0, 0, 0, 2, 0, 0, 0, 2, 0}, normals[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  static float radius[3] = {0.1f, 0.1f, 0.1f}, texcoords[6] = {0, 0, 1, 0, 0, 1}, other_texcoords[6] = {0, 0, 0.5f, 0, 0, 0.5f};
  static int   triangle[3] = {0, 1, 2}, other_triangle[3] = {0, 2, 1}, line[2] = {0, 1};
  yd::flat_scene base;
  yh_shape       sh{};
  sh.num_vertices = 3, sh.positions = positions, sh.normals = normals, sh.texcoords = texcoords, sh.num_triangles = 1, sh.triangles = triangle;
  base.shapes = {sh, sh, sh};
  base.shapes[2].num_triangles = 0, base.shapes[2].triangles = nullptr, base.shapes[2].num_lines = 1, base.shapes[2].lines = line, base.shapes[2].texcoords = nullptr;
  base.shape_vertex_edits = {0, 0, 0};
  yh_material grey{}, lamp{};
  grey.color[0] = grey.color[1] = grey.color[2] = 0.5f, grey.opacity = 1, grey.ior = 1.5f, grey.trdepth = 0.01f;
  lamp = grey, lamp.emission[0] = lamp.emission[1] = lamp.emission[2] = 5;
  base.materials = {grey, lamp};
  base.maps.assign(2, yh_material_maps{});
  yh_object ob{};
  ob.frame[0] = ob.frame[4] = ob.frame[8] = 1;
  base.objects = {ob, ob, ob};  // shape 0 under the lamp, shapes 1 and 2 grey
  base.objects[0].material = 1, base.objects[1].shape = 1, base.objects[2].shape = 2;
  yh_environment env{};
  env.frame[0] = env.frame[4] = env.frame[8] = 1, env.emission[0] = env.emission[1] = env.emission[2] = 0.5f;
  base.environments = {env};
  base.camera.frame[0] = base.camera.frame[4] = base.camera.frame[8] = 1, base.camera.lens = 0.05f, base.camera.film[0] = 0.036f, base.camera.film[1] = 0.024f;
  base.camera.focus = 10000;

  CHECK(yd::classify_edit(base, base, false, true) == yd::edit_none);
  // a position edit: as ever without the opt-in (through every overload), edit_shapes with it
  auto now = base;
  now.shapes[1].positions = other_positions;
  CHECK(yd::classify_edit(base, now) == yd::edit_upload && yd::classify_edit(base, now, false) == yd::edit_upload && yd::classify_edit(base, now, true) == yd::edit_upload);
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_shapes);
  CHECK(yd::shape_vertices_differ(base, now, 1) && !yd::shape_vertices_differ(base, now, 0) && !yd::shape_vertices_differ(base, now, 2));
  // ... the other vertex arrays, and the line shape's radius
  now = base, now.shapes[1].texcoords = other_texcoords;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_shapes && yd::classify_edit(base, now) == yd::edit_upload);
  now = base, now.shapes[2].radius = radius;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_shapes);
  // a setter that wrote into the same storage: seen by its count with the opt-in, and not looked at without (as ever)
  now = base, now.shape_vertex_edits[2] = 1;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_shapes && yd::shape_vertices_differ(base, now, 2));
  CHECK(yd::classify_edit(base, now) == yd::edit_none && yd::classify_edit(base, now, true) == yd::edit_none);
  // next to the edits the other calls take
  now = base, now.shapes[1].positions = other_positions, now.camera.focus = 3, now.objects[2].frame[9] = 1;
  CHECK(yd::classify_edit(base, now, true, true) == (yd::edit_shapes | yd::edit_camera | yd::edit_objects));
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);  // (the object's frame, without its opt-in)
  // edit_upload again as soon as a count or an index differs
  now = base, now.shapes[1].positions = other_positions, now.shapes[1].num_vertices = 2;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  now = base, now.shapes[1].positions = other_positions, now.shapes[1].triangles = other_triangle;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  now = base, now.shapes[1].triangles = other_triangle;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  now = base, now.shapes[2].num_lines = 2;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  // ... as normals or texcoords appear or vanish, and for the geometry of an emitter
  now = base, now.shapes[1].normals = nullptr;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  now = base, now.shapes[2].texcoords = texcoords;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  now = base, now.shapes[0].positions = other_positions;
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_upload);
  // without the opt-in everything else is as before
  now = base, now.camera.focus = 3;
  CHECK(yd::classify_edit(base, now, false, false) == yd::edit_camera && yd::classify_edit(base, now, false, true) == yd::edit_camera);
}

struct Built {
  std::unique_ptr<ptr::scene> scene = std::make_unique<ptr::scene>();
  ptr::camera*                camera = nullptr;
  ptr::shape*                 hair = nullptr;
};
static Built build(const yh_scene_file* file, const ptr::trace_params& params, bool opt_in) {
  Built b;
  b.camera = init_scene(b.scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
  for (auto& s : b.scene->shapes)
    if (!s->lines.empty()) b.hair = s.get();
  ptr::set_shape_edits(b.scene.get(), opt_in);
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
// a shear of the strands, x += 0.2 y^2, with the radii halved
static void comb(ptr::shape* hair) {
  auto positions = hair->positions;  // (copies of the same size: the setters write into the shape's own storage)
  auto radius    = hair->radius;
  for (auto& p : positions) p.x += 0.2f * p.y * p.y;
  for (auto& r : radius) r *= 0.5f;
  ptr::set_positions(hair, positions);
  ptr::set_radius(hair, radius);
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

    Built a    = build(file, params, true);
    auto  img0 = render(a, params);
    CHECK(a.hair != nullptr);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 0);
    const auto* storage = a.hair->positions.data();
    comb(a.hair);
    CHECK(a.hair->positions.data() == storage);  // the case pointers alone do not show
    auto img_combed = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1);
    CHECK(!same(img_combed, img0));
    auto again = render(a, params);  // nothing changed since: nothing happens
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1 && same(again, img_combed));

    // the same scene built with the combed hair from the start
    Built b = build(file, params, false);
    comb(b.hair);
    CHECK(same(render(b, params), img_combed));
    CHECK(b.scene->uploads == 1 && b.scene->edits == 0);
    // without the opt-in a vertex array that moved is the whole upload, as before
    auto moved = b.hair->positions;  // (a vector of its own, handed over: the shape's storage is another from here on)
    ptr::set_positions(b.hair, std::move(moved));
    render(b, params);
    CHECK(b.scene->uploads == 2 && b.scene->edits == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
