// tests/test_temporal_cli.py: the mirror's accumulate_image (an extension, host/yhair_pathtrace.h) over camera edits returns what the host's
// form yh_reproject makes of the state's image, the planes of trace_gbuffer and the previous call's result — with denoise parameters that
// image through yh_atrous_filter — keeps its history across the edits init_state passes on, and leaves the render as it was.
//   test_mirror_temporal <scene.json>
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

    std::vector<vec4f> hist_rgba;
    std::vector<int>   hist_length, hist_object;
    std::vector<vec3f> hist_position;
    yh_camera          hist_camera{};
    for (int step = 0; step < 3; step++) {
      if (step > 0) camera->frame.o.x += 0.02f * step, params.seed += 1;  // an edit init_state passes on as yh_update_camera
      ptr::state st;
      ptr::init_state(&st, scene.get(), camera, params);
      ptr::trace_samples(&st, scene.get(), camera, params, 4);
      const auto      render = st.render;
      const size_t    n      = (size_t)st.width * st.height;
      const auto      g      = ptr::trace_gbuffer(&st, scene.get(), camera, params);
      const yh_camera now    = scene->uploaded.camera;
      const auto      tp     = ptr::default_temporal_params();
      const auto      dp     = ptr::default_denoise_params();
      CHECK(tp.max_history >= 1 && tp.sigma_position > 0 && tp.match_object == 1);
      const bool denoised = step == 2;
      const auto img      = ptr::accumulate_image(&st, scene.get(), camera, params, tp, denoised ? &dp : nullptr);
      CHECK(img.width == st.width && img.height == st.height && img.pixels.size() == n);
      // the host's form on what the mirror hands out
      std::vector<vec4f> want(n);
      std::vector<int>   want_length(n), got_length(n);
      CHECK(yh_reproject(st.width, st.height, &tp, (const float*)render.data(), 4, g.object.pixels.data(), (const float*)g.position.pixels.data(),
                step ? (const float*)hist_rgba.data() : nullptr, step ? hist_length.data() : nullptr, step ? hist_object.data() : nullptr,
                step ? (const float*)hist_position.data() : nullptr, &now, step ? &hist_camera : nullptr, 0, nullptr, nullptr, nullptr, (float*)want.data(),
                want_length.data()) == YH_OK);
      CHECK(yh_temporal_lengths(yhair::detail::context(), got_length.data()) == (int)n);
      CHECK(got_length == want_length);
      auto shown = want;
      if (denoised)
        CHECK(yh_atrous_filter(st.width, st.height, &dp, (const float*)want.data(), g.object.pixels.data(), (const float*)g.normal.pixels.data(),
                  (const float*)g.position.pixels.data(), (const float*)g.albedo.pixels.data(), (float*)shown.data()) == YH_OK);
      CHECK(!memcmp(img.pixels.data(), shown.data(), n * sizeof(vec4f)));
      if (step == 0) CHECK(!memcmp(img.pixels.data(), render.data(), n * sizeof(vec4f)));  // the first frame passes through
      if (step > 0) {
        size_t reused = 0;
        for (size_t i = 0; i < n; i++) reused += want_length[i] > 4;
        CHECK(reused > n / 4);
      }
      CHECK(st.samples == 4 && !memcmp(st.render.data(), render.data(), n * sizeof(vec4f)));
      hist_rgba = want, hist_length = want_length, hist_object = g.object.pixels, hist_position = g.position.pixels, hist_camera = now;
    }
    CHECK(scene->uploads == 1 && scene->edits == 2);
    ptr::reset_accumulation();
    CHECK(yh_temporal_lengths(yhair::detail::context(), nullptr) == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
