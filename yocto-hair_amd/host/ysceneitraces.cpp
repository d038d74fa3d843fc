// ysceneitraces — the reference's progressive path tracer (apps/ysceneitraces/ysceneitraces.cpp) without its
// window: the OTHER caller of trace_samples, through the same C++ mirror (yhair_pathtrace.h).
//
// What it restates is reset_display (ysceneitraces.cpp:255-300), the only part of the app that touches the
// path: init_state of the render state; a PREVIEW state at resolution / pratio traced for one sample and
// upscaled into the display image; then an asynchronous worker that calls the stop-flag overload of
// trace_samples once per sample (pt.cpp:2009-2026) until the samples are done or the flag is set — which is
// what a camera edit does in the app and what --stop-after-ms does here.
//
// Same flags as the app (ysceneitraces.cpp:313-327): --camera, --resolution,-r, --samples,-s, --shader,-t,
// --bounces,-b, --clamp, --output,-o, positional scene. Extensions: --pratio (trace_params::pratio, default
// 8), --preview-image FILE, --stop-after-ms N, --seed, --device, --gpus / --devices, --features PREFIX [--features-mode centre|next] (the first-hit
// feature pass after the preview: yscene_cli.h, save_features), --denoise FILE (the preview pass denoised: save_denoised), --sway STEPS [--sway-refit] (the vertex edit's gesture: the first
// line shape displaced step by step, passed on through yh_update_shape or, with --sway-refit, yh_refit_shape) and --turntable STEPS: the app's one gesture, the
// camera orbit (ysceneitraces.cpp:392-410: update_turntable on app->camera->frame, then reset_display), headless — after the first
// reset_display, STEPS - 1 times a rotation by 2 pi / STEPS followed by reset_display again; step k is saved as <stem>-<kkk><ext>.
#include <atomic>
#include <chrono>
#include <cmath>
#include <future>
#include <thread>

#include "yscene_cli.h"

// update_turntable for a frame parametrization with a rotation only (yocto_math.h:5072-5085) and the lookat_frame it calls (:3229-3239)
static vec3f operator-(const vec3f& a, const vec3f& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static vec3f operator+(const vec3f& a, const vec3f& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static vec3f operator*(const vec3f& a, float b) { return {a.x * b, a.y * b, a.z * b}; }
static vec3f cross(const vec3f& a, const vec3f& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static float length(const vec3f& a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
static vec3f normalize(const vec3f& a) {
  auto l = length(a);
  return (l != 0) ? vec3f{a.x / l, a.y / l, a.z / l} : a;
}
static frame3f lookat_frame(const vec3f& eye, const vec3f& center, const vec3f& up) {
  auto w = normalize(eye - center);
  auto u = normalize(cross(up, w));
  auto v = normalize(cross(w, u));
  return {u, v, w, eye};
}
static void update_turntable(frame3f& frame, float& focus, const vec2f& rotate) {
  if (rotate.x == 0 && rotate.y == 0) return;
  const float pif = (float)3.14159265358979323846;
  auto phi   = std::atan2(frame.z.z, frame.z.x) + rotate.x;
  auto theta = std::acos(frame.z.y) + rotate.y;
  theta      = std::min(std::max(theta, 0.001f), pif - 0.001f);
  auto new_z = vec3f{std::sin(theta) * std::cos(phi), std::cos(theta), std::sin(theta) * std::sin(phi)};
  auto new_center = frame.o - frame.z * focus;
  auto new_o      = new_center + new_z * focus;
  frame           = lookat_frame(new_o, new_center, {0, 1, 0});
  focus           = length(new_o - new_center);
}

int main(int argc, const char* argv[]) {
  auto        params = ptr::trace_params{};
  std::string camera_name, imagename = "out.hdr", preview_name, filename, shader = "path", features, features_mode_name = "centre", denoise, temporal, variance;
  int         stop_after_ms = -1, gpus = 1, first_device = 0, turntable = 0;
  bool        turn_objects = false, sway_refit = false, variance_guided = false;
  int         sway = 0;
  std::string device_list;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) print_fatal("missing value for " + a);
      return argv[++i];
    };
    if (a == "--help" || a == "-h") {
      printf("usage: ysceneitraces [--camera NAME] [--resolution,-r N] [--samples,-s N] [--shader,-t naive|path|eyelight|normal]\n"
             "                     [--bounces,-b N] [--clamp F] [--output,-o FILE] [--pratio N] [--preview-image FILE]\n"
             "                     [--stop-after-ms N] [--seed N] [--device N] [--gpus N] [--devices A,B,..] [--turntable STEPS [--turntable-objects]]\n"
             "                     [--sway STEPS [--sway-refit]] [--features PREFIX] [--features-mode centre|next] [--denoise FILE]\n"
             "                     [--temporal FILE [--variance-guided] [--variance FILE]] scene\n"
             "Progressive path tracing of hair scenes on MI355X (headless: preview pass, then samples until done or stopped)\n");
      return 0;
    } else if (a == "--camera") camera_name = next();
    else if (a == "--resolution" || a == "-r") params.resolution = atoi(next().c_str());
    else if (a == "--samples" || a == "-s") params.samples = atoi(next().c_str());
    else if (a == "--shader" || a == "-t") shader = next();
    else if (a == "--bounces" || a == "-b") params.bounces = atoi(next().c_str());
    else if (a == "--clamp") params.clamp = (float)atof(next().c_str());
    else if (a == "--output" || a == "-o") imagename = next();
    else if (a == "--pratio") params.pratio = std::max(1, atoi(next().c_str()));
    else if (a == "--preview-image") preview_name = next();
    else if (a == "--stop-after-ms") stop_after_ms = atoi(next().c_str());
    else if (a == "--seed") params.seed = strtoull(next().c_str(), nullptr, 10);
    else if (a == "--device") first_device = atoi(next().c_str());
    else if (a == "--gpus") gpus = std::max(1, atoi(next().c_str()));
    else if (a == "--devices") device_list = next();
    else if (a == "--turntable") turntable = std::max(1, atoi(next().c_str()));
    else if (a == "--turntable-objects") turn_objects = true;
    else if (a == "--sway") sway = std::max(1, atoi(next().c_str()));
    else if (a == "--sway-refit") sway_refit = true;
    else if (a == "--features") features = next();
    else if (a == "--features-mode") features_mode_name = next();
    else if (a == "--denoise") denoise = next();
    else if (a == "--temporal") temporal = next();
    else if (a == "--variance-guided") variance_guided = true;
    else if (a == "--variance") variance = next();
    else if (!a.empty() && a[0] == '-') print_fatal("unknown option " + a);
    else filename = a;
  }
  if (filename.empty()) print_fatal("missing scene");
  if (turn_objects && turntable <= 0) print_fatal("--turntable-objects needs --turntable STEPS");
  if (sway_refit && sway <= 0) print_fatal("--sway-refit needs --sway STEPS");
  if (sway > 0 && turntable > 0) print_fatal("--sway and --turntable are gestures of their own");
  if (!temporal.empty() && turntable <= 0) print_fatal("--temporal needs --turntable STEPS");
  if (variance_guided && (temporal.empty() || denoise.empty())) print_fatal("--variance-guided needs --temporal FILE and --denoise FILE");
  if (!variance.empty() && temporal.empty()) print_fatal("--variance needs --temporal FILE");
  if (!temporal.empty()) params.pratio = 1;  // (the history lives at one image size: the preview pass has the render's)
  yh_set_trial_cache_dir(yh_default_trial_cache_dir());  // the command line keeps its kernel-trial record on disk (include/yhair.h); a library caller has to ask
  set_devices(first_device, gpus, device_list);
  bool known = false;
  for (size_t i = 0; i < ptr::shader_names.size(); i++)
    if (ptr::shader_names[i] == shader) params.shader = (ptr::shader_type)i, known = true;
  if (!known) print_fatal("unknown shader " + shader);
  const auto feature_mode = features_mode(features_mode_name);

  try {
    char error[512];
    auto ioscene = yh_scene_load(filename.c_str(), camera_name.c_str(), error, sizeof(error));
    if (!ioscene) print_fatal(error);
    auto scene  = std::make_unique<ptr::scene>();
    auto camera = init_scene(scene.get(), yh_scene_get(ioscene), yh_scene_get_maps(ioscene));
    yh_scene_free(ioscene);
    ptr::init_bvh(scene.get(), params);
    ptr::init_lights(scene.get(), params);

    // ---- reset_display (ysceneitraces.cpp:255-300) -------------------------------------------------------
    std::chrono::steady_clock::time_point t_edit;  // --turntable: when the camera was moved
    auto reset_display = [&](const std::string& imagename, bool orbit, bool last = true) {
    const int uploads0 = scene->uploads;
    auto render_state = std::make_unique<ptr::state>();
    ptr::init_state(render_state.get(), scene.get(), camera, params);
    const int          W = render_state->width, H = render_state->height;
    std::vector<vec4f> render((size_t)W * H);  // app->render: what the window shows
    // render preview
    auto t0     = std::chrono::steady_clock::now();
    auto pstate = std::make_unique<ptr::state>();
    auto pprms  = params;
    pprms.resolution /= params.pratio;
    pprms.samples = 1;
    ptr::init_state(pstate.get(), scene.get(), camera, pprms);
    ptr::trace_samples(pstate.get(), scene.get(), camera, pprms);
    for (int j = 0; j < H; j++)
      for (int i = 0; i < W; i++) {
        int pi = std::min(std::max(i / params.pratio, 0), pstate->width - 1), pj = std::min(std::max(j / params.pratio, 0), pstate->height - 1);
        render[(size_t)j * W + i] = pstate->render[(size_t)pj * pstate->width + pi];
      }
    printf("preview: %dx%d at 1 spp upscaled to %dx%d, %.1f ms\n", pstate->width, pstate->height, W, H,
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (orbit && sway > 0)
      printf("sway step, edit to preview: %.1f ms (%s)\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_edit).count(),
          scene->uploads > uploads0 ? "the scene was uploaded again" : sway_refit ? "the hair alone was passed on, as a refit" : "the hair alone was passed on, its tree built again");
    else if (orbit)
      printf("edit to preview: %.1f ms (%s)\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_edit).count(),
          scene->uploads > uploads0 ? "the scene was uploaded again" : turn_objects ? "the objects alone were passed on" : "the camera alone was passed on");
    if (!preview_name.empty() && yh_save_image(preview_name.c_str(), W, H, (const float*)render.data(), error, sizeof(error)) != YH_OK)
      print_fatal(error);
    if (!denoise.empty() && temporal.empty()) save_denoised(pstate.get(), scene.get(), camera, pprms, denoise);  // (yscene_cli.h: the 1-spp preview denoised, at the preview's resolution)
    if (!features.empty()) save_features(render_state.get(), scene.get(), camera, params, features, feature_mode);  // (yscene_cli.h; binds the render state again)
    // start render
    std::atomic<bool> render_stop{false};
    std::atomic<int>  render_counter{0};
    auto t1            = std::chrono::steady_clock::now();
    auto render_worker = std::async(std::launch::async, [&]() {
      for (int sample = 0; sample < params.samples; sample++) {
        ptr::trace_samples(render_state.get(), scene.get(), camera, params, &render_stop);
        if (render_stop) return;
        render = render_state->render;
        render_counter = sample + 1;
      }
    });
    if (stop_after_ms >= 0) {  // the user moves the camera: reset_display sets the flag and waits for the worker
      std::this_thread::sleep_for(std::chrono::milliseconds(stop_after_ms));
      render_stop = true;
    }
    render_worker.get();
    auto dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    printf("render: %d of %d samples in %.3fs%s\n", (int)render_counter, params.samples, dt, render_stop ? " (stopped)" : "");
    if (yh_save_image(imagename.c_str(), W, H, (const float*)render.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
    printf("save image: %s\n", imagename.c_str());
    // --temporal FILE: this step's finished render joins the steps before it (yscene_cli.h: accumulate_step); the last step's accumulated
    // image is written, and with --denoise FILE that file holds it denoised — by the variance-guided levels with --variance-guided;
    // --variance FILE holds the last step's variance estimate
    if (!temporal.empty() && render_state->samples > 0) accumulate_step(render_state.get(), scene.get(), camera, params, temporal, denoise, last, variance_guided, variance);
    };
    if (sway > 0) {  // the vertex edit's gesture: step k displaces the first line shape by x += a_k y^2, a_k = 0.1 k / STEPS, tangents recomputed
      const size_t slash = imagename.find_last_of('/'), dot = imagename.find_last_of('.');
      const bool   ext   = dot != std::string::npos && (slash == std::string::npos || dot > slash);
      const std::string stem = ext ? imagename.substr(0, dot) : imagename, suffix = ext ? imagename.substr(dot) : "";
      ptr::shape* hair = nullptr;
      for (auto& s : scene->shapes)
        if (!hair && !s->lines.empty()) hair = s.get();
      if (!hair) print_fatal("--sway: the scene has no line shape");
      ptr::set_shape_edits(scene.get(), true);
      ptr::set_shape_refit(scene.get(), sway_refit);
      const std::vector<vec3f> loaded = hair->positions;
      for (int k = 0; k <= sway; k++) {
        if (k > 0) {
          t_edit = std::chrono::steady_clock::now();
          const float a = 0.1f * k / sway;
          std::vector<vec3f> positions = loaded, tangents(loaded.size(), vec3f{0, 0, 0});
          for (auto& p : positions) p.x += a * p.y * p.y;
          for (auto& l : hair->lines) {  // a vertex's tangent: the normalised sum of the directions of the segments at it
            const vec3f &p0 = positions[(size_t)l.x], &p1 = positions[(size_t)l.y], d = {p1.x - p0.x, p1.y - p0.y, p1.z - p0.z};
            for (int v : {l.x, l.y}) tangents[(size_t)v] = {tangents[(size_t)v].x + d.x, tangents[(size_t)v].y + d.y, tangents[(size_t)v].z + d.z};
          }
          for (auto& t : tangents) {
            const float len = std::sqrt(t.x * t.x + t.y * t.y + t.z * t.z);
            if (len > 0) t = {t.x / len, t.y / len, t.z / len};
          }
          ptr::set_positions(hair, positions);
          if (!hair->normals.empty()) ptr::set_normals(hair, tangents);
        }
        char number[16];
        snprintf(number, sizeof(number), "-%03d", k);
        reset_display(stem + number + suffix, k > 0);
      }
    } else if (turntable <= 0) {
      reset_display(imagename, false);
    } else {  // the orbit: one turn in `turntable` steps, step k saved as <stem>-<kkk><ext>
      const size_t slash = imagename.find_last_of('/'), dot = imagename.find_last_of('.');
      const bool   ext   = dot != std::string::npos && (slash == std::string::npos || dot > slash);
      const std::string stem = ext ? imagename.substr(0, dot) : imagename, suffix = ext ? imagename.substr(dot) : "";
      std::vector<std::pair<ptr::object*, frame3f>> turning;  // --turntable-objects: what turns, with its loaded frame
      if (turn_objects) {
        ptr::set_object_edits(scene.get(), true);
        for (auto& o : scene->objects) {
          const auto& e = o->material_->emission;
          if (e.x == 0 && e.y == 0 && e.z == 0) turning.push_back({o.get(), o->frame});
        }
      }
      for (int k = 0; k < turntable; k++) {
        if (k > 0 && turn_objects) {
          t_edit = std::chrono::steady_clock::now();
          const float a = 2 * (float)3.14159265358979323846 * k / turntable, c = std::cos(a), s = std::sin(a);
          auto turn = [&](const vec3f& v) { return vec3f{c * v.x + s * v.z, v.y, c * v.z - s * v.x}; };  // about the world's y axis
          for (auto& [o, f] : turning) ptr::set_frame(o, frame3f{turn(f.x), turn(f.y), turn(f.z), turn(f.o)});
        } else if (k > 0) {
          t_edit = std::chrono::steady_clock::now();
          update_turntable(camera->frame, camera->focus, {2 * (float)3.14159265358979323846 / turntable, 0});
        }
        char number[16];
        snprintf(number, sizeof(number), "-%03d", k);
        reset_display(stem + number + suffix, k > 0, k == turntable - 1);
      }
    }
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  return 0;
}
