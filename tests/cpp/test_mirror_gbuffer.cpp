// tests/test_gbuffer.py: the mirror's trace_gbuffer (an extension, host/yhair_pathtrace.h) returns the planes of the C ABI's
// yh_trace_gbuffer on the state's image, in both modes, and leaves the render as it would have been without it.
//   test_mirror_gbuffer <scene.json>
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

template <typename T>
static bool same(const std::vector<T>& a, const void* b, size_t n) {
  return a.size() == n && n > 0 && !memcmp(a.data(), b, n * sizeof(T));
}

int main(int argc, const char* argv[]) {
  if (argc < 2) return 2;
  try {
    char err[512] = "";
    auto file     = yh_scene_load(argv[1], "", err, sizeof(err));
    if (!file) print_fatal(err);
    auto params       = ptr::trace_params{};
    params.resolution = 60, params.samples = 2, params.shader = ptr::shader_type::normal;
    auto scene  = std::make_unique<ptr::scene>();
    auto camera = init_scene(scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
    ptr::init_bvh(scene.get(), params);
    ptr::init_lights(scene.get(), params);

    ptr::state plain;  // the render without the pass
    ptr::init_state(&plain, scene.get(), camera, params);
    ptr::trace_samples(&plain, scene.get(), camera, params, 2);
    const auto want = plain.render;

    ptr::state st;
    ptr::init_state(&st, scene.get(), camera, params);
    const size_t n = (size_t)st.width * st.height;
    for (auto mode : {ptr::gbuffer_mode::centre, ptr::gbuffer_mode::next_sample}) {
      const auto g = ptr::trace_gbuffer(&st, scene.get(), camera, params, mode);
      CHECK(g.object.width == st.width && g.object.height == st.height && g.ray.width == st.width && g.albedo.height == st.height);
      std::vector<int>   object(n), element(n), material(n);
      std::vector<float> uv(2 * n), distance(n), position(3 * n), normal(3 * n), tangent(3 * n), texcoord(2 * n), albedo(3 * n), ray(6 * n);
      yh_gbuffer out{object.data(), element.data(), material.data(), uv.data(), distance.data(), position.data(), normal.data(), tangent.data(),
          texcoord.data(), albedo.data(), ray.data()};
      CHECK(yh_trace_gbuffer(yhair::detail::context(), (int)mode, &out) == YH_OK);
      CHECK(same(g.object.pixels, object.data(), n) && same(g.element.pixels, element.data(), n) && same(g.material.pixels, material.data(), n));
      CHECK(same(g.uv.pixels, uv.data(), n) && same(g.distance.pixels, distance.data(), n) && same(g.position.pixels, position.data(), n));
      CHECK(same(g.normal.pixels, normal.data(), n) && same(g.tangent.pixels, tangent.data(), n) && same(g.texcoord.pixels, texcoord.data(), n));
      CHECK(same(g.albedo.pixels, albedo.data(), n) && same(g.ray.pixels, ray.data(), n));
      size_t hits = 0;
      for (size_t i = 0; i < n; i++) hits += object[i] >= 0;
      CHECK(hits > n / 10 && hits < n);
      CHECK((g.object[{st.width / 2, st.height / 2}]) == object[(size_t)(st.height / 2) * st.width + st.width / 2]);
    }
    ptr::trace_samples(&st, scene.get(), camera, params, 2);
    CHECK(st.samples == 2 && st.render.size() == want.size() && !memcmp(st.render.data(), want.data(), want.size() * sizeof(vec4f)));
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
