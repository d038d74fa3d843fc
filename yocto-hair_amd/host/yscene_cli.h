// yscene_cli.h — what the two command lines share: print_fatal (yocto_commonio.h:258-261) and init_scene, the
// conversion of a loaded scene into a ptr::scene through the public add_* / set_* API, as both of the
// reference's apps do (apps/yscenetrace/yscenetrace.cpp:49-197, apps/ysceneitraces/ysceneitraces.cpp:96-243).
#ifndef YSCENE_CLI_H_
#define YSCENE_CLI_H_
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "yhair_pathtrace.h"

namespace ptr = yhair::pathtrace;
using namespace yhair::math;

[[noreturn]] inline void print_fatal(const std::string& msg) {
  printf("%s\n", msg.c_str());
  exit(1);
}

// sio::model -> ptr::scene through the public scene-construction API, as
// init_scene does in the reference CLI (cli.cpp:49-197).
// `maps`: the materials' scalar and normal maps (yh_scene_get_maps), or NULL.
inline ptr::camera* init_scene(ptr::scene* scene, const yh_scene_desc* d, const yh_material_maps* maps = nullptr) {
  auto frame_of = [](const float* f) {
    frame3f r;
    memcpy(&r, f, 48);
    return r;
  };
  auto camera = ptr::add_camera(scene);
  ptr::set_frame(camera, frame_of(d->camera.frame));
  camera->lens = d->camera.lens, camera->film = {d->camera.film[0], d->camera.film[1]};
  ptr::set_focus(camera, d->camera.aperture, d->camera.focus);
  std::vector<ptr::texture*> textures;  // material textures and maps (yh_scene_desc::textures)
  for (int i = 0; i < d->num_textures; i++) {
    auto&  t = d->textures[i];
    auto   o = ptr::add_texture(scene);
    size_t n = (size_t)t.width * t.height;
    if (t.is_byte) {
      std::vector<yhair::pathtrace::vec3b> img(n);
      memcpy((void*)img.data(), t.pixels, 3 * n);
      ptr::set_texture(o, t.width, t.height, img);
    } else {
      std::vector<vec3f> img(n);
      memcpy((void*)img.data(), t.pixels, sizeof(float) * 3 * n);
      ptr::set_texture(o, t.width, t.height, img);
    }
    textures.push_back(o);
  }
  auto texture_of = [&](int id) { return id > 0 ? textures[(size_t)id - 1] : nullptr; };
  std::vector<ptr::material*> materials;
  for (int i = 0; i < d->num_materials; i++) {
    auto& m = d->materials[i];
    auto  o = ptr::add_material(scene);
    ptr::set_eumelanin(o, m.eumelanin), ptr::set_pheomelanin(o, m.pheomelanin);
    ptr::set_sigma_a(o, {m.sigma_a[0], m.sigma_a[1], m.sigma_a[2]});
    ptr::set_beta_m(o, m.beta_m), ptr::set_beta_n(o, m.beta_n), ptr::set_alpha(o, m.alpha), ptr::set_eta(o, m.eta);
    ptr::set_emission(o, vec3f{m.emission[0], m.emission[1], m.emission[2]}, texture_of(m.emission_tex));
    ptr::set_color(o, {m.color[0], m.color[1], m.color[2]}, texture_of(m.color_tex));
    const yh_material_maps mm = maps ? maps[i] : yh_material_maps{};
    ptr::set_specular(o, m.specular, texture_of(mm.specular_tex)), ptr::set_ior(o, m.ior);
    ptr::set_metallic(o, m.metallic, texture_of(mm.metallic_tex));
    ptr::set_transmission(o, m.transmission, m.thin != 0, m.trdepth, texture_of(mm.transmission_tex));
    ptr::set_scattering(o, {m.scattering[0], m.scattering[1], m.scattering[2]}, m.scanisotropy, texture_of(m.scattering_tex));
    ptr::set_roughness(o, m.roughness, texture_of(mm.roughness_tex)), ptr::set_opacity(o, m.opacity, texture_of(mm.opacity_tex));
    ptr::set_thin(o, m.thin != 0), ptr::set_normalmap(o, texture_of(mm.normal_tex));
    materials.push_back(o);
  }
  std::vector<ptr::shape*> shapes;
  for (int i = 0; i < d->num_shapes; i++) {
    auto& s = d->shapes[i];
    auto  o = ptr::add_shape(scene);
    auto  v3 = [](const float* p, int n) {  // (one pass: no zero fill before the copy)
      static_assert(sizeof(vec3f) == 12, "vec3f is three floats");
      const vec3f* q = (const vec3f*)p;
      return std::vector<vec3f>(q, q + n);
    };
    ptr::set_positions(o, v3(s.positions, s.num_vertices));
    if (s.normals) ptr::set_normals(o, v3(s.normals, s.num_vertices));
    if (s.radius) ptr::set_radius(o, std::vector<float>(s.radius, s.radius + s.num_vertices));
    if (s.texcoords) {
      std::vector<yhair::pathtrace::vec2f> tc((size_t)s.num_vertices);
      memcpy((void*)tc.data(), s.texcoords, sizeof(float) * 2 * (size_t)s.num_vertices);
      ptr::set_texcoords(o, tc);
    }
    if (s.num_lines) ptr::set_lines(o, std::vector<vec2i>((const vec2i*)s.lines, (const vec2i*)s.lines + s.num_lines));
    if (s.num_triangles) ptr::set_triangles(o, std::vector<vec3i>((const vec3i*)s.triangles, (const vec3i*)s.triangles + s.num_triangles));
    shapes.push_back(o);
  }
  for (int i = 0; i < d->num_objects; i++) {
    auto o = ptr::add_object(scene);
    ptr::set_frame(o, frame_of(d->objects[i].frame));
    ptr::set_shape(o, shapes[d->objects[i].shape]);
    ptr::set_material(o, materials[d->objects[i].material]);
  }
  for (int i = 0; i < d->num_environments; i++) {
    auto& e = d->environments[i];
    auto  o = ptr::add_environment(scene);
    ptr::set_frame(o, frame_of(e.frame));
    ptr::texture* tex = nullptr;
    if (e.texels) {
      tex = ptr::add_texture(scene);
      std::vector<vec3f> img((size_t)e.tex_width * e.tex_height);
      memcpy(img.data(), e.texels, sizeof(float) * 3 * img.size());
      ptr::set_texture(tex, e.tex_width, e.tex_height, img);
    }
    ptr::set_emission(o, {e.emission[0], e.emission[1], e.emission[2]}, tex);
  }
  return camera;
}

// "--devices a,b,c" / "--gpus N": the devices the contexts are made on (yhair_pathtrace.h: detail::devices())
inline void set_devices(int first, int gpus, const std::string& list) {
  auto& devs = yhair::detail::devices();
  devs.clear();
  if (!list.empty()) {
    size_t at = 0;
    while (at <= list.size()) {
      size_t comma = list.find(',', at);
      if (comma == std::string::npos) comma = list.size();
      devs.push_back(atoi(list.substr(at, comma - at).c_str()));
      at = comma + 1;
    }
  } else {
    for (int i = 0; i < (gpus < 1 ? 1 : gpus); i++) devs.push_back(first + i);
  }
}

// "--features PREFIX [--features-mode centre|next]" (an extension of both command lines): the first-hit feature pass over the state's image
// (ptr::trace_gbuffer; context 0 alone runs it, whatever --gpus says) as four images — PREFIX.normal.hdr = normal * 0.5 + 0.5 as the `normal`
// shader shows it, PREFIX.albedo.hdr, PREFIX.depth.hdr = the distance in all three channels, PREFIX.ids.hdr = object, element, material as
// floats; a pixel that hits nothing is 0 in all four (RGBE holds no negative value). The ids file is a picture of the masks, not a table: RGBE
// keeps eight bits of a pixel's largest channel, so a large element id rounds the object and material ids next to it; exact ids come from
// the C ABI or the mirror
inline ptr::gbuffer_mode features_mode(const std::string& name) {
  if (name == "centre") return ptr::gbuffer_mode::centre;
  if (name == "next") return ptr::gbuffer_mode::next_sample;
  print_fatal("unknown features mode " + name);
}
inline void save_features(ptr::state* state, const ptr::scene* scene, const ptr::camera* camera, const ptr::trace_params& params, const std::string& prefix,
    ptr::gbuffer_mode mode) {
  const auto g = ptr::trace_gbuffer(state, scene, camera, params, mode);
  const size_t n = (size_t)state->width * state->height;
  std::vector<yhair::math::vec4f> img(n);
  char error[512];
  auto save = [&](const char* what) {
    const std::string name = prefix + "." + what + ".hdr";
    if (yh_save_image(name.c_str(), state->width, state->height, (const float*)img.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
    printf("save features: %s\n", name.c_str());
  };
  for (size_t i = 0; i < n; i++) {
    const auto& v = g.normal.pixels[i];
    const bool  hit = g.object.pixels[i] >= 0;
    img[i] = hit ? yhair::math::vec4f{v.x * 0.5f + 0.5f, v.y * 0.5f + 0.5f, v.z * 0.5f + 0.5f, 1} : yhair::math::vec4f{0, 0, 0, 1};
  }
  save("normal");
  for (size_t i = 0; i < n; i++) img[i] = {g.albedo.pixels[i].x, g.albedo.pixels[i].y, g.albedo.pixels[i].z, 1};
  save("albedo");
  for (size_t i = 0; i < n; i++) img[i] = {g.distance.pixels[i], g.distance.pixels[i], g.distance.pixels[i], 1};
  save("depth");
  for (size_t i = 0; i < n; i++) img[i] = {(float)g.object.pixels[i], (float)g.element.pixels[i], (float)g.material.pixels[i], 1};
  save("ids");
}
// "--denoise FILE" (an extension of both command lines): the state's image denoised with the library's default parameters
// (ptr::denoise_image: from the gathered image on context 0, whatever --gpus says), written next to the untouched output
inline void save_denoised(ptr::state* state, const ptr::scene* scene, const ptr::camera* camera, const ptr::trace_params& params, const std::string& name) {
  const auto img = ptr::denoise_image(state, scene, camera, params, ptr::default_denoise_params());
  char       error[512];
  if (yh_save_image(name.c_str(), img.width, img.height, (const float*)img.pixels.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
  printf("save denoised: %s\n", name.c_str());
}
// "--temporal FILE" (an extension of ysceneitraces --turntable): every step's finished render is accumulated over the steps
// (ptr::accumulate_image with the library's default parameters, on context 0 whatever --gpus says); at the last step the accumulated
// image is written to `name` and, with --denoise FILE given too, denoised (the library's defaults) to `denoised_name`
inline void accumulate_step(ptr::state* state, const ptr::scene* scene, const ptr::camera* camera, const ptr::trace_params& params, const std::string& name,
    const std::string& denoised_name, bool last, bool variance_guided = false, const std::string& variance_name = "") {
  if (variance_guided || !variance_name.empty()) {
    // "--variance-guided" / "--variance FILE": the steps accumulate with the variance stage's moments beside the colour
    // (ptr::accumulate_image_variance, the library's defaults); at the last step the accumulated image goes to `name`, the variance estimate
    // as a grey image to `variance_name`, and `denoised_name` holds the accumulated image through the variance-guided levels
    // (--variance-guided) or through yh_denoise's
    const auto         vp = ptr::default_variance_params();
    std::vector<float> var;
    auto               img = ptr::accumulate_image_variance(state, scene, camera, params, ptr::default_temporal_params(), vp, &var, false);
    if (!last) return;
    char error[512];
    if (yh_save_image(name.c_str(), img.width, img.height, (const float*)img.pixels.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
    printf("save accumulated: %s\n", name.c_str());
    if (!variance_name.empty()) {
      std::vector<vec4f> grey(var.size());
      for (size_t i = 0; i < var.size(); i++) grey[i] = {var[i], var[i], var[i], 1.0f};
      if (yh_save_image(variance_name.c_str(), img.width, img.height, (const float*)grey.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
      printf("save variance: %s\n", variance_name.c_str());
    }
    if (denoised_name.empty()) return;
    const auto dp = ptr::default_denoise_params();
    const int  rc = variance_guided ? yh_denoise_variance_image(yhair::detail::context(), &vp, (const float*)img.pixels.data(), nullptr, nullptr, (float*)img.pixels.data(), nullptr)
                                    : yh_denoise(yhair::detail::context(), &dp, (const float*)img.pixels.data(), (float*)img.pixels.data());
    if (rc != YH_OK) print_fatal("the filter of the accumulated image failed");
    if (yh_save_image(denoised_name.c_str(), img.width, img.height, (const float*)img.pixels.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
    printf("save accumulated and denoised: %s\n", denoised_name.c_str());
    return;
  }
  auto img = ptr::accumulate_image(state, scene, camera, params, ptr::default_temporal_params());
  if (!last) return;
  char error[512];
  if (yh_save_image(name.c_str(), img.width, img.height, (const float*)img.pixels.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
  printf("save accumulated: %s\n", name.c_str());
  if (denoised_name.empty()) return;
  const auto dp = ptr::default_denoise_params();
  if (yh_denoise(yhair::detail::context(), &dp, (const float*)img.pixels.data(), (float*)img.pixels.data()) != YH_OK) print_fatal("yh_denoise of the accumulated image failed");
  if (yh_save_image(denoised_name.c_str(), img.width, img.height, (const float*)img.pixels.data(), error, sizeof(error)) != YH_OK) print_fatal(error);
  printf("save accumulated and denoised: %s\n", denoised_name.c_str());
}
#endif
