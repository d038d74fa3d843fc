// tests/test_denoise_cli.py: the mirror's denoise_image (an extension, host/yhair_pathtrace.h) returns what the C ABI's yh_denoise makes
// of the state's image, with the library's defaults and with parameters of the caller's, and leaves the render as it would have been
// without it.
//   test_mirror_denoise <scene.json>
// Exit status 0 and "ok" on success; a failed check prints its line.
#include "yscene_cli.h"

static int failures = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) printf("line %d: %s\n", __LINE__, #x), failures++; \
  } while (0)

int main(int argc, const char* argv[]) {
  if (argc < 2) return 2;
  try {
    char err[512] = "";
    auto file     = yh_scene_load(argv[1], "", err, sizeof(err));
    if (!file) print_fatal(err);
    auto params       = ptr::trace_params{};
    params.resolution = 60, params.samples = 4;
    auto scene  = std::make_unique<ptr::scene>();
    auto camera = init_scene(scene.get(), yh_scene_get(file), yh_scene_get_maps(file));
    ptr::init_bvh(scene.get(), params);
    ptr::init_lights(scene.get(), params);

    ptr::state plain;  // the render without the calls
    ptr::init_state(&plain, scene.get(), camera, params);
    ptr::trace_samples(&plain, scene.get(), camera, params, 2);
    ptr::trace_samples(&plain, scene.get(), camera, params, 2);
    const auto want = plain.render;

    ptr::state st;
    ptr::init_state(&st, scene.get(), camera, params);
    ptr::trace_samples(&st, scene.get(), camera, params, 2);
    const auto   half = st.render;
    const size_t n    = (size_t)st.width * st.height;
    auto         dp   = ptr::default_denoise_params();
    CHECK(dp.iterations == 5 && dp.sigma_position > 0 && dp.demodulate == 1);
    auto loose         = dp;
    loose.iterations   = 2, loose.match_object = 0, loose.demodulate = 0;
    for (const auto& p : {dp, loose}) {
      const auto img = ptr::denoise_image(&st, scene.get(), camera, params, p);
      CHECK(img.width == st.width && img.height == st.height && img.pixels.size() == n);
      std::vector<float> abi(4 * n);
      CHECK(yh_denoise(yhair::detail::context(), &p, nullptr, abi.data()) == YH_OK);  // (one device: the own render is the downloaded one)
      CHECK(!memcmp(img.pixels.data(), abi.data(), n * sizeof(vec4f)));
      CHECK(memcmp(img.pixels.data(), half.data(), n * sizeof(vec4f)) != 0);
      CHECK(st.samples == 2 && !memcmp(st.render.data(), half.data(), n * sizeof(vec4f)));
    }
    ptr::trace_samples(&st, scene.get(), camera, params, 2);
    CHECK(st.samples == 4 && st.render.size() == want.size() && !memcmp(st.render.data(), want.data(), want.size() * sizeof(vec4f)));
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
