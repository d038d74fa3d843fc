// tests/test_shape_refit.py: the mirror's second opt-in (set_shape_refit, an extension). Together with set_shape_edits, a shape's
// positions, normals, radius or texcoords set after an init_state go through yh_refit_shape at the next one — seen through
// yh_shape_refit_growth, which a build leaves at exactly 1 — and with set_shape_refit alone nothing changes: the edit is the whole
// upload, as ever. How an edit is classified depends on neither (detail::classify_edit does not know the flag).
//   test_mirror_shape_refit --classify       the flags and the classification alone: no device needed
//   test_mirror_shape_refit <scene.json>     then renders on the device
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

namespace yd = yhair::detail;

static void classification() {
  ptr::scene sc;
  CHECK(!sc.shape_refit && !sc.shape_edits);  // off by default
  ptr::set_shape_refit(&sc, true);
  CHECK(sc.shape_refit && !sc.shape_edits);  // an opt-in of its own: it does not switch the vertex edits on
  static float positions[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, other_positions[9] = {0, 0, 0, 2, 0, 0, 0, 2, 0};
  static int   line[2] = {0, 1};
  yd::flat_scene base;
  yh_shape       sh{};
  sh.num_vertices = 3, sh.positions = positions, sh.num_lines = 1, sh.lines = line;
  base.shapes = {sh};
  base.shape_vertex_edits = {0};
  yh_material grey{};
  grey.color[0] = grey.color[1] = grey.color[2] = 0.5f, grey.opacity = 1, grey.ior = 1.5f, grey.trdepth = 0.01f;
  base.materials = {grey};
  base.maps.assign(1, yh_material_maps{});
  yh_object ob{};
  ob.frame[0] = ob.frame[4] = ob.frame[8] = 1;
  base.objects = {ob};
  base.camera.frame[0] = base.camera.frame[4] = base.camera.frame[8] = 1, base.camera.lens = 0.05f, base.camera.film[0] = 0.036f, base.camera.film[1] = 0.024f;
  auto now = base;
  now.shapes[0].positions = other_positions;
  // the default classification: a vertex edit without set_shape_edits is the upload, with it edit_shapes; the signature took no new flag
  CHECK(yd::classify_edit(base, now) == yd::edit_upload && yd::classify_edit(base, now, false, false) == yd::edit_upload);
  CHECK(yd::classify_edit(base, now, false, true) == yd::edit_shapes);
}

struct Built {
  std::unique_ptr<ptr::scene> scene = std::make_unique<ptr::scene>();
  ptr::camera*                camera = nullptr;
  ptr::shape*                 hair = nullptr;
  int                         hair_index = -1;
};
static Built build(const yh_scene_file* file, const ptr::trace_params& params, bool edits, bool refit) {
  Built b;
  b.camera = init_scene(b.scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
  for (size_t i = 0; i < b.scene->shapes.size(); i++)
    if (!b.scene->shapes[i]->lines.empty()) b.hair = b.scene->shapes[i].get(), b.hair_index = (int)i;
  ptr::set_shape_edits(b.scene.get(), edits);
  ptr::set_shape_refit(b.scene.get(), refit);
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
// a shear of the strands, x += 0.2 y^2
static void comb(ptr::shape* hair) {
  auto positions = hair->positions;
  for (auto& p : positions) p.x += 0.2f * p.y * p.y;
  ptr::set_positions(hair, positions);
}
static bool grew(const Built& b) {
  float g[3] = {0, 0, 0};
  CHECK(yh_shape_refit_growth(yd::require_context(), b.hair_index, g) == YH_OK);
  return g[0] != 1.0f || g[1] != 1.0f || g[2] != 1.0f;
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

    // both opt-ins: one upload, one edit, and the boxes of the tree that stayed have grown
    Built a = build(file, params, true, true);
    render(a, params);
    CHECK(a.hair != nullptr && a.scene->uploads == 1 && a.scene->edits == 0 && !grew(a));
    comb(a.hair);
    auto img_refit = render(a, params);
    CHECK(a.scene->uploads == 1 && a.scene->edits == 1 && grew(a));

    // set_shape_edits alone: the same edit is a build (growth exactly 1)
    Built b = build(file, params, true, false);
    render(b, params);
    comb(b.hair);
    auto img_built = render(b, params);
    CHECK(b.scene->uploads == 1 && b.scene->edits == 1 && !grew(b));
    CHECK(img_refit.size() == img_built.size() && !img_built.empty());

    // set_shape_refit alone: nothing changes, the edit is the whole upload
    Built c = build(file, params, false, true);
    render(c, params);
    auto moved = c.hair->positions;  // (a vector of its own, handed over: without set_shape_edits only another storage shows an edit)
    for (auto& p : moved) p.x += 0.2f * p.y * p.y;
    ptr::set_positions(c.hair, std::move(moved));
    render(c, params);
    CHECK(c.scene->uploads == 2 && c.scene->edits == 0 && !grew(c));
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
