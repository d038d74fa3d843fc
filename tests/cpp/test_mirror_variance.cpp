// tests/test_variance_cli.py: the mirror's accumulate_image_variance (an extension, host/yhair_pathtrace.h) over camera edits returns what
// the host's forms yh_reproject_moments, yh_variance_spatial and yh_atrous_variance_filter make of the state's image, the planes of
// trace_gbuffer and the previous call's result; a plain accumulate_image in between starts the moments afresh; the render stays as it was.
//   test_mirror_variance <scene.json>
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
    std::vector<int>   hist_length, hist_object, hist_steps;
    std::vector<vec3f> hist_position;
    std::vector<float> hist_moments;
    yh_camera          hist_camera{};
    for (int step = 0; step < 4; step++) {
      if (step > 0) camera->frame.o.x += 0.02f * step, params.seed += 1;  // an edit init_state passes on as yh_update_camera
      ptr::state st;
      ptr::init_state(&st, scene.get(), camera, params);
      ptr::trace_samples(&st, scene.get(), camera, params, 4);
      const auto      render = st.render;
      const size_t    n      = (size_t)st.width * st.height;
      const auto      g      = ptr::trace_gbuffer(&st, scene.get(), camera, params);
      const yh_camera now    = scene->uploaded.camera;
      const auto      tp     = ptr::default_temporal_params();
      const auto      vp     = ptr::default_variance_params();
      CHECK(vp.iterations >= 1 && vp.sigma_luminance > 0 && vp.epsilon > 0 && vp.min_steps >= 1 && vp.demodulate == 1);
      const bool         plain = step == 2;  // a plain accumulate in between: the colour goes on, the moments are marked as none
      std::vector<float> got_variance;
      const auto         img = plain ? ptr::accumulate_image(&st, scene.get(), camera, params, tp)
                                     : ptr::accumulate_image_variance(&st, scene.get(), camera, params, tp, vp, &got_variance);
      CHECK(img.width == st.width && img.height == st.height && img.pixels.size() == n);
      // the host's forms on what the mirror hands out
      const bool         moments = step > 0 && !hist_steps.empty();
      std::vector<vec4f> acc(n), want(n);
      std::vector<int>   want_length(n), want_steps(n), got(n);
      std::vector<float> want_moments(2 * n), var(n), want_variance(n);
      CHECK(yh_reproject_moments(st.width, st.height, &tp, (const float*)render.data(), 4, g.object.pixels.data(), (const float*)g.position.pixels.data(),
                (const float*)g.albedo.pixels.data(), step ? (const float*)hist_rgba.data() : nullptr, step ? hist_length.data() : nullptr,
                step ? hist_object.data() : nullptr, step ? (const float*)hist_position.data() : nullptr, moments ? hist_moments.data() : nullptr,
                moments ? hist_steps.data() : nullptr, &now, step ? &hist_camera : nullptr, 0, nullptr, nullptr, nullptr, (float*)acc.data(), want_length.data(),
                want_moments.data(), want_steps.data()) == YH_OK);
      CHECK(yh_temporal_lengths(yhair::detail::context(), got.data()) == (int)n);
      CHECK(got == want_length);
      if (plain) {
        CHECK(!memcmp(img.pixels.data(), acc.data(), n * sizeof(vec4f)));
        CHECK(yh_temporal_steps(yhair::detail::context(), nullptr) == 0);
        hist_steps.clear(), hist_moments.clear();
      } else {
        CHECK(yh_variance_spatial(st.width, st.height, &tp, vp.min_steps, want_moments.data(), want_steps.data(), g.object.pixels.data(),
                  (const float*)g.position.pixels.data(), var.data()) == YH_OK);
        CHECK(yh_atrous_variance_filter(st.width, st.height, &vp, (const float*)acc.data(), var.data(), g.object.pixels.data(), (const float*)g.normal.pixels.data(),
                  (const float*)g.position.pixels.data(), (const float*)g.albedo.pixels.data(), (float*)want.data(), want_variance.data()) == YH_OK);
        CHECK(!memcmp(img.pixels.data(), want.data(), n * sizeof(vec4f)));
        CHECK(got_variance.size() == n && !memcmp(got_variance.data(), want_variance.data(), n * sizeof(float)));
        CHECK(yh_temporal_steps(yhair::detail::context(), got.data()) == (int)n);
        CHECK(got == want_steps);
        int longest = 0;
        for (size_t i = 0; i < n; i++) longest = want_steps[i] > longest ? want_steps[i] : longest;
        CHECK(longest == (step == 1 ? 2 : 1));  // steps 0 and 3 start the moments, step 1 carries them on
        hist_steps = want_steps, hist_moments = want_moments;
      }
      CHECK(st.samples == 4 && !memcmp(st.render.data(), render.data(), n * sizeof(vec4f)));
      hist_rgba = acc, hist_length = want_length, hist_object = g.object.pixels, hist_position = g.position.pixels, hist_camera = now;
    }
    CHECK(scene->uploads == 1 && scene->edits == 3);
    ptr::reset_accumulation();
    CHECK(yh_temporal_steps(yhair::detail::context(), nullptr) == 0 && yh_temporal_lengths(yhair::detail::context(), nullptr) == 0);
    yh_scene_free(file);
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  if (failures) return 11;
  printf("ok\n");
  return 0;
}
