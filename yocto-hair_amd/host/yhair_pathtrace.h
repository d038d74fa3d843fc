// yhair_pathtrace.h — host-side C++ mirror of the reference's interface for the
// hair path, implemented on top of the C ABI (include/yhair.h).
//
// Same names, argument meaning and error behaviour as
//   yocto::pathtrace  (libs/yocto_pathtrace/yocto_pathtrace.h:97-230): add_* /
//     set_* scene construction, trace_params, init_bvh, init_lights,
//     init_state, trace_samples;
//   yocto::extension  (libs/yocto_extension/yocto_extension.h:84-130):
//     hair_material, hair_brdf, eval_hair_brdf, eval_hair_scattering,
//     sample_hair_scattering, sample_hair_scattering_pdf (and its README name
//     eval_hair_scattering_pdf), and the four self-tests, which print "OK!" or
//     throw std::runtime_error("TEST FAILED!") exactly like the reference.
// so that a caller of the reference's API (apps/yscenetrace/yscenetrace.cpp:
// 241-258) switches by changing the namespace. All arithmetic runs on the GPU:
// these functions only marshal arguments. Programmer errors throw
// std::runtime_error (as pt.cpp:1669 does); there is no CPU fallback.
#ifndef YHAIR_PATHTRACE_H_
#define YHAIR_PATHTRACE_H_
#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "yhair.h"

namespace yhair::math {
struct vec2f { float x = 0, y = 0; };
struct vec2i { int x = 0, y = 0; };
struct vec3f { float x = 0, y = 0, z = 0; };
struct vec3i { int x = 0, y = 0, z = 0; };
struct vec4f { float x = 0, y = 0, z = 0, w = 0; };
struct frame3f {
  vec3f x = {1, 0, 0}, y = {0, 1, 0}, z = {0, 0, 1}, o = {0, 0, 0};
};
}  // namespace yhair::math

namespace yhair::detail {
// The devices the path runs on: one context per entry (default: device 0). With more than one, the image's
// 8x8 tiles are dealt round-robin to the contexts (yh_set_shard), every context renders all samples of its own
// tiles from its own host thread, and the framebuffer is gathered over RCCL (yh_gather_framebuffer). Pixel
// results do not depend on the number of GPUs. Set before the first call that needs a context.
inline std::vector<int>& devices() {
  static std::vector<int> devs = {0};
  return devs;
}
inline int& device() { return devices()[0]; }
inline std::vector<yh_context*>& contexts() {
  static std::vector<yh_context*> ctxs;
  return ctxs;
}
inline std::vector<yh_context*>& require_contexts() {
  auto& ctxs = contexts();
  if (ctxs.empty()) {
    for (int dev : devices()) {
      auto ctx = yh_create(dev);
      if (!ctx) throw std::runtime_error(std::string("yhair: ") + yh_last_error(nullptr));
      ctxs.push_back(ctx);
    }
  }
  return ctxs;
}
inline yh_context* require_context() { return require_contexts()[0]; }
inline yh_context* context() { return contexts().empty() ? nullptr : contexts()[0]; }
inline void check(int rc, yh_context* ctx = nullptr) {
  if (rc != YH_OK) throw std::runtime_error(std::string("yhair: ") + yh_last_error(ctx ? ctx : context()));
}
// fn(context, index) on every context, each from its own host thread (calls of the C ABI block)
template <typename F>
inline void for_each_context(F&& fn) {
  auto& ctxs = require_contexts();
  if (ctxs.size() == 1) {
    check(fn(ctxs[0], 0), ctxs[0]);
    return;
  }
  std::vector<int>         rcs(ctxs.size(), YH_OK);
  std::vector<std::thread> pool;
  for (size_t i = 0; i < ctxs.size(); i++) pool.emplace_back([&, i]() { rcs[i] = fn(ctxs[i], (int)i); });
  for (auto& t : pool) t.join();
  for (size_t i = 0; i < ctxs.size(); i++) check(rcs[i], ctxs[i]);
}
// A scene graph flattened to the C ABI's description: what an upload passes, and what the scene remembers of its last one.
struct flat_scene {
  std::vector<yh_shape>         shapes;  // per shape its pointers and counts
  std::vector<yh_material>      materials;
  std::vector<yh_material_maps> maps;
  std::vector<yh_object>        objects;
  std::vector<yh_environment>   environments;
  std::vector<yh_texture>       textures;
  std::vector<unsigned>         shape_vertex_edits;  // per shape how often a vertex setter ran (shape::vertex_edits); empty: all 0
  yh_camera                     camera{};
  yh_scene_desc desc() const {
    yh_scene_desc d{};
    d.num_shapes = (int)shapes.size(), d.shapes = shapes.data();
    d.num_materials = (int)materials.size(), d.materials = materials.data();
    d.num_objects = (int)objects.size(), d.objects = objects.data();
    d.num_environments = (int)environments.size(), d.environments = environments.data();
    d.num_textures = (int)textures.size(), d.textures = textures.data();
    d.camera = camera;
    return d;
  }
};
// What separates the description a scene last uploaded from the one it flattens to now: a set of edit_camera / edit_materials /
// edit_environments — exactly the differences yh_update_camera / yh_update_materials / yh_update_environments accept
// (include/yhair.h) — or edit_upload as soon as anything else differs: a shape's pointers or counts, an object (its frame too), a
// texture, a map, the number of anything, a material's texture ids, an emission that turns on or off. No device, no context.
// objects_too (EXTENSION, see set_object_edits): objects that differ in frame or material only are edit_objects, what
// yh_update_objects accepts, unless the new material turns the object's emission on or off; an object's shape stays edit_upload.
// shapes_too (EXTENSION, see set_shape_edits): a shape whose counts and index arrays are the uploaded ones and which differs in
// positions, normals, radius or texcoords only — by their pointers, or by a vertex setter having run since the upload, which writes
// into the same storage when the sizes agree — is edit_shapes, what yh_update_shape accepts, unless normals or texcoords appear or
// vanish or an object that names it emits (its light tables were made from it). Without it nothing of this is looked at.
// lights_too (EXTENSION, see set_light_edits): what changes the light list no longer makes an edit an upload — a material or an
// environment whose emission turns on or off, an object whose new material does, the vertex arrays of an emitter's shape (with
// shapes_too) — since yh_set_light_edits makes the yh_update_* calls take them. The default classification is unchanged.
enum : unsigned { edit_none = 0, edit_camera = 1, edit_materials = 2, edit_environments = 4, edit_upload = 8, edit_objects = 16, edit_shapes = 32 };
// whether shape i differs in its vertex arrays alone (the counts and the index arrays being equal is the caller's business)
inline bool shape_vertices_differ(const flat_scene& was, const flat_scene& now, size_t i) {
  const yh_shape &a = was.shapes[i], &b = now.shapes[i];
  auto edits = [i](const flat_scene& f) { return i < f.shape_vertex_edits.size() ? f.shape_vertex_edits[i] : 0u; };
  return a.positions != b.positions || a.normals != b.normals || a.radius != b.radius || a.texcoords != b.texcoords || edits(was) != edits(now);
}
inline unsigned classify_edit(const flat_scene& was, const flat_scene& now, bool objects_too, bool shapes_too = false, bool lights_too = false) {
  auto black = [](const float* e) { return e[0] == 0 && e[1] == 0 && e[2] == 0; };
  if (was.shapes.size() != now.shapes.size() || was.materials.size() != now.materials.size() || was.maps.size() != now.maps.size() ||
      was.objects.size() != now.objects.size() || was.environments.size() != now.environments.size() || was.textures.size() != now.textures.size())
    return edit_upload;
  unsigned shape_kind = edit_none;
  for (size_t i = 0; i < now.shapes.size(); i++) {
    const yh_shape &a = was.shapes[i], &b = now.shapes[i];
    if (a.num_vertices != b.num_vertices || a.num_lines != b.num_lines || a.lines != b.lines || a.num_triangles != b.num_triangles || a.triangles != b.triangles)
      return edit_upload;
    if (!shapes_too) {
      if (a.positions != b.positions || a.normals != b.normals || a.radius != b.radius || a.texcoords != b.texcoords) return edit_upload;
      continue;
    }
    if (!shape_vertices_differ(was, now, i)) continue;
    if (!b.positions || (a.normals != nullptr) != (b.normals != nullptr) || (a.texcoords != nullptr) != (b.texcoords != nullptr)) return edit_upload;
    for (size_t o = 0; o < now.objects.size() && !lights_too; o++) {  // an emitter's geometry: the light list was made from it
      const yh_object& ob = now.objects[o];
      if ((size_t)ob.shape == i && ob.material >= 0 && (size_t)ob.material < now.materials.size() && !black(now.materials[(size_t)ob.material].emission)) return edit_upload;
    }
    shape_kind = edit_shapes;
  }
  for (size_t i = 0; i < now.textures.size(); i++) {
    const yh_texture &a = was.textures[i], &b = now.textures[i];
    if (a.width != b.width || a.height != b.height || a.is_byte != b.is_byte || a.pixels != b.pixels) return edit_upload;
  }
  unsigned kind = shape_kind;
  for (size_t i = 0; i < now.objects.size(); i++) {
    const yh_object &a = was.objects[i], &b = now.objects[i];
    if (a.shape != b.shape) return edit_upload;
    if (!memcmp(a.frame, b.frame, 48) && a.material == b.material) continue;
    if (!objects_too) return edit_upload;
    const size_t nm = now.materials.size();
    if (a.material < 0 || b.material < 0 || (size_t)a.material >= nm || (size_t)b.material >= nm) return edit_upload;
    if (!lights_too && black(was.materials[(size_t)a.material].emission) != black(now.materials[(size_t)b.material].emission)) return edit_upload;  // the light list changes
    kind |= edit_objects;
  }
  static_assert(sizeof(yh_material_maps) == 6 * sizeof(int) && sizeof(yh_material) == 30 * 4 && sizeof(yh_camera) == 17 * 4, "compared as bytes: no padding");
  if (!now.maps.empty() && memcmp(was.maps.data(), now.maps.data(), sizeof(yh_material_maps) * now.maps.size())) return edit_upload;
  for (size_t i = 0; i < now.materials.size(); i++) {
    const yh_material &a = was.materials[i], &b = now.materials[i];
    if (!memcmp(&a, &b, sizeof(a))) continue;
    if ((!lights_too && black(a.emission) != black(b.emission)) || a.emission_tex != b.emission_tex || a.color_tex != b.color_tex || a.scattering_tex != b.scattering_tex) return edit_upload;
    kind |= edit_materials;
  }
  for (size_t i = 0; i < now.environments.size(); i++) {
    const yh_environment &a = was.environments[i], &b = now.environments[i];
    if (a.tex_width != b.tex_width || a.tex_height != b.tex_height || a.texels != b.texels || (!lights_too && black(a.emission) != black(b.emission))) return edit_upload;
    if (memcmp(a.frame, b.frame, 48) || memcmp(a.emission, b.emission, 12)) kind |= edit_environments;
  }
  if (memcmp(&was.camera, &now.camera, sizeof(yh_camera))) kind |= edit_camera;
  return kind;
}
inline unsigned classify_edit(const flat_scene& was, const flat_scene& now) { return classify_edit(was, now, false); }
// the state whose pixels the contexts hold (see init_state / trace_samples)
inline const void*& bound_state() {
  static const void* st = nullptr;
  return st;
}
}  // namespace yhair::detail

// -----------------------------------------------------------------------------
namespace yhair::extension {
using math::frame3f;
using math::vec2f;
using math::vec3f;

inline const int p_max = 3;
struct hair_material {  // ext.h:86-95
  vec3f sigma_a     = {0, 0, 0};
  float beta_m      = 0.3f;
  float beta_n      = 0.3f;
  float alpha       = 2;
  float eta         = 1.55f;
  vec3f color       = {0, 0, 0};
  float eumelanin   = 0;
  float pheomelanin = 0;
};
struct hair_brdf {  // ext.h:97-113 (30 floats, same field order)
  vec3f                        sigma_a = {0, 0, 0};
  float                        alpha   = 2;
  float                        eta     = 1.55f;
  float                        h       = 0;
  std::array<float, p_max + 1> v       = {};
  float                        s       = 0;
  vec3f                        sin_2k_alpha, cos_2k_alpha;
  float                        gamma_o = 0;
  frame3f                      world_to_brdf;
};
static_assert(sizeof(hair_brdf) == sizeof(float) * YH_HAIR_BRDF_FLOATS, "hair_brdf layout");

inline yh_material to_material(const hair_material& m) {
  yh_material o{};
  o.opacity = 1, o.ior = 1.5f, o.thin = 1, o.trdepth = 0.01f;
  o.sigma_a[0] = m.sigma_a.x, o.sigma_a[1] = m.sigma_a.y, o.sigma_a[2] = m.sigma_a.z;
  o.beta_m = m.beta_m, o.beta_n = m.beta_n, o.alpha = m.alpha, o.eta = m.eta;
  o.color[0] = m.color.x, o.color[1] = m.color.y, o.color[2] = m.color.z;
  o.eumelanin = m.eumelanin, o.pheomelanin = m.pheomelanin;
  return o;
}
inline hair_brdf eval_hair_brdf(const hair_material& material, float v, const vec3f& normal, const vec3f& tangent) {
  auto      m = to_material(material);
  hair_brdf b;
  detail::check(yh_hair_brdf_batch(detail::require_context(), 1, &m, &v, &normal.x, &tangent.x, (float*)&b));
  return b;
}
inline vec3f eval_hair_scattering(const hair_brdf& brdf, const vec3f& outgoing, const vec3f& incoming) {
  vec3f f;
  detail::check(yh_hair_eval_batch(detail::require_context(), 1, (const float*)&brdf, &outgoing.x, &incoming.x, &f.x));
  return f;
}
inline vec3f sample_hair_scattering(const hair_brdf& brdf, const vec3f& outgoing, const vec2f& rn) {
  vec3f w;
  detail::check(yh_hair_sample_batch(detail::require_context(), 1, (const float*)&brdf, &outgoing.x, &rn.x, &w.x));
  return w;
}
inline float sample_hair_scattering_pdf(const hair_brdf& brdf, const vec3f& outgoing, const vec3f& incoming) {
  float pdf = 0;
  detail::check(yh_hair_pdf_batch(detail::require_context(), 1, (const float*)&brdf, &outgoing.x, &incoming.x, &pdf));
  return pdf;
}
// README.md:20 names it eval_hair_scattering_pdf
inline float eval_hair_scattering_pdf(const hair_brdf& brdf, const vec3f& outgoing, const vec3f& incoming) {
  return sample_hair_scattering_pdf(brdf, outgoing, incoming);
}
inline void run_selftest(int which) {
  auto rc = yh_selftest(detail::require_context(), which, nullptr);
  if (rc == YH_E_SELFTEST) throw std::runtime_error("TEST FAILED!");  // ext.cpp:582
  detail::check(rc);
  printf("OK!\n");
  fflush(stdout);
}
inline void white_furnace_test() { run_selftest(0); }
inline void white_furnace_sampled_test() { run_selftest(1); }
inline void sampling_weights_test() { run_selftest(2); }
inline void sampling_consistency_test() { run_selftest(3); }
}  // namespace yhair::extension

// -----------------------------------------------------------------------------
namespace yhair::pathtrace {
using math::frame3f;
using math::vec2f;
using math::vec2i;
using math::vec3f;
using math::vec3i;
using math::vec4f;

struct vec3b { unsigned char x = 0, y = 0, z = 0; };
struct texture {  // pt.h:282-287: colorf / colorb; a scalar image (scalarf / scalarb) is kept as grey RGB, which lookup_texture treats alike (pt.cpp:147-164)
  int                width = 0, height = 0;
  std::vector<vec3f> colorf;
  std::vector<vec3b> colorb;
};
struct camera {  // pt.h:272-278
  frame3f frame;
  float   lens     = 0.050f;
  vec2f   film     = {0.036f, 0.024f};
  float   focus    = 10000;
  float   aperture = 0;
};
struct material {  // pt.h:293-329
  vec3f emission = {0, 0, 0}, color = {0, 0, 0};
  texture *emission_tex = nullptr, *color_tex = nullptr, *scattering_tex = nullptr;
  texture *specular_tex = nullptr, *metallic_tex = nullptr, *roughness_tex = nullptr, *transmission_tex = nullptr;
  texture *opacity_tex = nullptr, *normal_tex = nullptr;
  float specular = 0, roughness = 0, metallic = 0, ior = 1.5f, transmission = 0, opacity = 1;
  bool  thin = false;
  vec3f scattering = {0, 0, 0};
  float scanisotropy = 0, trdepth = 0.01f;
  float eumelanin = 0, pheomelanin = 0;
  vec3f sigma_a = {0, 0, 0};
  float beta_m = 0.3f, beta_n = 0.3f, alpha = 2, eta = 1.55f;
};
struct shape {  // pt.h:335-366
  std::vector<vec2i> lines;
  std::vector<vec3i> triangles;
  std::vector<vec3f> positions, normals;
  std::vector<vec2f> texcoords;
  std::vector<float> radius;
  unsigned           vertex_edits = 0;  // EXTENSION: how often set_positions / _normals / _radius / _texcoords ran (see set_shape_edits)
};
struct object {
  frame3f   frame;
  shape*    shape_   = nullptr;
  material* material_ = nullptr;
};
struct environment {
  frame3f  frame;
  vec3f    emission     = {0, 0, 0};
  texture* emission_tex = nullptr;
};
struct scene {
  std::vector<std::unique_ptr<camera>>      cameras;
  std::vector<std::unique_ptr<object>>      objects;
  std::vector<std::unique_ptr<shape>>       shapes;
  std::vector<std::unique_ptr<material>>    materials;
  std::vector<std::unique_ptr<texture>>     textures;
  std::vector<std::unique_ptr<environment>> environments;
  // set by init_bvh / init_lights, consumed by init_state (which knows the camera)
  mutable bool          bvh_requested = false, lights_requested = false;
  mutable const camera* uploaded_for  = nullptr;
  mutable double        upload_seconds = 0;  // wall-clock of the last flatten + yh_upload_scene (init_bvh + init_lights of the reference), for the command line's --timing
  // What the scene last uploaded, flattened: init_state compares it with the scene as it is now, so that an edit made through the set_*
  // functions after an init_state takes effect as it does in the reference, which reads these structs live (see init_state). How many
  // init_state calls uploaded the whole scene and how many only passed edits on:
  mutable detail::flat_scene uploaded;
  mutable int                uploads = 0, edits = 0;
  bool                       object_edits = false;  // EXTENSION (set_object_edits): object frames and materials go through yh_update_objects
  bool                       shape_edits  = false;  // EXTENSION (set_shape_edits): vertex edits of a shape go through yh_update_shape
  bool                       shape_refit  = false;  // EXTENSION (set_shape_refit): ... through yh_refit_shape instead
  bool                       light_edits  = false;  // EXTENSION (set_light_edits): what changes the light list is an edit too (yh_set_light_edits)
};
struct state {  // pt.h:426-429; `render` is refreshed by trace_samples
  int                width = 0, height = 0, samples = 0;
  std::vector<vec4f> render;
  yh_trace_params    device_params{};  // what init_state asked for (see trace_samples: re-binding)
};
enum struct shader_type { naive, path, eyelight, normal };
const auto default_seed = 961748941ull;
struct trace_params {  // pt.h:188-197
  int         resolution = 720;
  shader_type shader     = shader_type::path;
  int         samples    = 512;
  int         bounces    = 8;
  float       clamp      = 100;
  uint64_t    seed       = default_seed;
  bool        noparallel = false;
  int         pratio     = 8;
  bool        hair_exact = false;  // extension: the hair BSDF's exact arithmetic (yh_trace_params::hair_exact)
};
const auto shader_names = std::vector<std::string>{"naive", "path", "eyelight", "normal"};
using progress_callback = std::function<void(const std::string& message, int current, int total)>;

// scene construction (pt.h:97-174)
inline camera*      add_camera(scene* s) { return s->cameras.emplace_back(new camera{}).get(); }
inline object*      add_object(scene* s) { return s->objects.emplace_back(new object{}).get(); }
inline texture*     add_texture(scene* s) { return s->textures.emplace_back(new texture{}).get(); }
inline material*    add_material(scene* s) { return s->materials.emplace_back(new material{}).get(); }
inline shape*       add_shape(scene* s) { return s->shapes.emplace_back(new shape{}).get(); }
inline environment* add_environment(scene* s) { return s->environments.emplace_back(new environment{}).get(); }
inline void set_frame(camera* c, const frame3f& f) { c->frame = f; }
inline void set_lens(camera* c, float lens, float aspect, float film) {  // pt.cpp:2088-2092
  c->lens = lens;
  c->film = aspect >= 1 ? vec2f{film, film / aspect} : vec2f{film * aspect, film};
}
inline void set_focus(camera* c, float aperture, float focus) { c->aperture = aperture, c->focus = focus; }
inline void set_frame(object* o, const frame3f& f) { o->frame = f; }
inline void set_material(object* o, material* m) { o->material_ = m; }
inline void set_shape(object* o, shape* s) { o->shape_ = s; }
inline void set_texture(texture* t, int width, int height, const std::vector<vec3f>& img) {
  t->width = width, t->height = height, t->colorf = img;
}
inline void set_eumelanin(material* m, float v) { m->eumelanin = v; }
inline void set_pheomelanin(material* m, float v) { m->pheomelanin = v; }
inline void set_sigma_a(material* m, vec3f v) { m->sigma_a = v; }
inline void set_beta_m(material* m, float v) { m->beta_m = v; }
inline void set_beta_n(material* m, float v) { m->beta_n = v; }
inline void set_alpha(material* m, float v) { m->alpha = v; }
inline void set_eta(material* m, float v) { m->eta = v; }
inline void set_texture(texture* t, int width, int height, const std::vector<vec3b>& img) {
  t->width = width, t->height = height, t->colorb = img, t->colorf.clear();
}
// scalar images (pt.h:117-118), expanded to grey RGB
inline void set_texture(texture* t, int width, int height, const std::vector<float>& img) {
  t->width = width, t->height = height, t->colorb.clear(), t->colorf.resize(img.size());
  for (size_t i = 0; i < img.size(); i++) t->colorf[i] = {img[i], img[i], img[i]};
}
inline void set_texture(texture* t, int width, int height, const std::vector<unsigned char>& img) {
  t->width = width, t->height = height, t->colorf.clear(), t->colorb.resize(img.size());
  for (size_t i = 0; i < img.size(); i++) t->colorb[i] = {img[i], img[i], img[i]};
}
inline void set_emission(material* m, const vec3f& e, texture* tex = nullptr) { m->emission = e, m->emission_tex = tex; }
inline void set_color(material* m, const vec3f& c, texture* tex = nullptr) { m->color = c, m->color_tex = tex; }
inline void set_texcoords(shape* s, const std::vector<vec2f>& v) { s->texcoords = v, s->vertex_edits++; }
inline void set_specular(material* m, float v = 1, texture* tex = nullptr) { m->specular = v, m->specular_tex = tex; }
inline void set_ior(material* m, float v) { m->ior = v; }
inline void set_metallic(material* m, float v, texture* tex = nullptr) { m->metallic = v, m->metallic_tex = tex; }
inline void set_transmission(material* m, float t, bool thin, float trdepth, texture* tex = nullptr) {
  m->transmission = t, m->thin = thin, m->trdepth = trdepth, m->transmission_tex = tex;
}
inline void set_scattering(material* m, const vec3f& scattering, float scanisotropy, texture* tex = nullptr) {
  m->scattering = scattering, m->scanisotropy = scanisotropy, m->scattering_tex = tex;
}
inline void set_roughness(material* m, float v, texture* tex = nullptr) { m->roughness = v, m->roughness_tex = tex; }
inline void set_opacity(material* m, float v, texture* tex = nullptr) { m->opacity = v, m->opacity_tex = tex; }
inline void set_normalmap(material* m, texture* tex) { m->normal_tex = tex; }
inline void set_thin(material* m, bool thin) { m->thin = thin; }
inline void set_lines(shape* s, const std::vector<vec2i>& v) { s->lines = v; }
inline void set_triangles(shape* s, const std::vector<vec3i>& v) { s->triangles = v; }
inline void set_positions(shape* s, const std::vector<vec3f>& v) { s->positions = v, s->vertex_edits++; }
inline void set_normals(shape* s, const std::vector<vec3f>& v) { s->normals = v, s->vertex_edits++; }
inline void set_radius(shape* s, const std::vector<float>& v) { s->radius = v, s->vertex_edits++; }
// (the same taking a temporary: the reference's signatures copy; a caller that hands over a vector it no longer needs — a loader — moves it: 60 MB for a hair model)
inline void set_lines(shape* s, std::vector<vec2i>&& v) { s->lines = std::move(v); }
inline void set_triangles(shape* s, std::vector<vec3i>&& v) { s->triangles = std::move(v); }
inline void set_positions(shape* s, std::vector<vec3f>&& v) { s->positions = std::move(v), s->vertex_edits++; }
inline void set_normals(shape* s, std::vector<vec3f>&& v) { s->normals = std::move(v), s->vertex_edits++; }
inline void set_radius(shape* s, std::vector<float>&& v) { s->radius = std::move(v), s->vertex_edits++; }
inline void set_frame(environment* e, const frame3f& f) { e->frame = f; }
// EXTENSION (no reference counterpart: the reference reads every struct live and has nothing to opt into). By default an object whose
// frame or material changed since the last init_state costs the whole upload at the next one; with `on`, such objects are passed on
// through yh_update_objects, which keeps every shape's tree and builds the scene-level tree again (include/yhair.h). What that call
// refuses — an object's shape, emission on or off, a tree too deep, a scene level that changes its form — falls back to the upload.
inline void set_object_edits(scene* s, bool on) { s->object_edits = on; }
// EXTENSION, off by default like the one above. With `on`, a shape whose positions, normals (the hair tangents), radius or texcoords were
// set since the last init_state — its counts and its lines / triangles being the uploaded ones — is passed on through yh_update_shape:
// that shape's tree, records and nodes are made again, no other shape, texture or light table is touched (include/yhair.h). What that
// call refuses — an emitter's geometry, a tree too deep, a scene level that changes its form — falls back to the upload.
inline void set_shape_edits(scene* s, bool on) { s->shape_edits = on; }
// EXTENSION, off by default, with effect only together with set_shape_edits(s, true): the vertex edits that opt-in passes on — counts and
// index arrays being the uploaded ones — go through yh_refit_shape instead of yh_update_shape: the shape keeps the tree of its last
// build and gets its records and boxes again (include/yhair.h: REFIT; closest hits those of a build, ties apart; yh_shape_refit_growth
// tells what the boxes grew by). How an edit is classified does not change, nor what falls back to the upload.
inline void set_shape_refit(scene* s, bool on) { s->shape_refit = on; }
// EXTENSION, off by default. With `on`, init_state passes on as an edit what changes the LIGHT LIST (include/yhair.h: LIGHT EDITS): an
// emission turned on or off by a material setter or by set_emission on an environment, set_material on an object under
// set_object_edits, and a vertex edit of an emitter's shape under set_shape_edits / set_shape_refit. The contexts make the light list
// again on the device. What they still refuse — a 17th light, no light left (also in between: the materials are passed on before the
// environments), another texture — falls back to the upload.
inline void set_light_edits(scene* s, bool on) { s->light_edits = on; }
inline void set_emission(environment* e, const vec3f& em, texture* tex = nullptr) { e->emission = em, e->emission_tex = tex; }

// Flattens the scene graph into a yh_scene_desc and uploads it; the C ABI builds
// the BVHs (init_bvh, pt.cpp:755-818) and the lights (init_lights,
// pt.cpp:1695-1740) in that one call. The camera is part of the uploaded scene,
// so the upload happens in init_state, the first call that receives it.
inline detail::flat_scene flatten_scene(const scene* sc, const camera* cam) {
  detail::flat_scene flat;
  auto &shapes = flat.shapes;
  auto &materials = flat.materials;
  auto &maps = flat.maps;
  auto &objects = flat.objects;
  auto &envs = flat.environments;
  auto &textures = flat.textures;
  std::vector<int>            texture_slot(sc->textures.size(), 0);  // 1-based slot in `textures`, 0 = not a material texture
  auto material_texture = [&](const texture* t) -> int {
    if (!t) return 0;
    for (size_t i = 0; i < sc->textures.size(); i++) {
      if (sc->textures[i].get() != t) continue;
      if (!texture_slot[i]) {
        yh_texture o{};
        o.width = t->width, o.height = t->height, o.is_byte = t->colorf.empty();
        o.pixels = o.is_byte ? (const void*)t->colorb.data() : (const void*)t->colorf.data();
        textures.push_back(o);
        texture_slot[i] = (int)textures.size();
      }
      return texture_slot[i];
    }
    throw std::runtime_error("yhair: material references a texture that is not in the scene");
  };
  auto index_of = [](auto& vec, auto* p) {
    for (size_t i = 0; i < vec.size(); i++)
      if (vec[i].get() == p) return (int)i;
    throw std::runtime_error("yhair: object references a shape/material that is not in the scene");
  };
  for (auto& s : sc->shapes) {
    yh_shape o{};
    o.num_vertices  = (int)s->positions.size();
    o.positions     = (const float*)s->positions.data();
    o.normals       = s->normals.empty() ? nullptr : (const float*)s->normals.data();
    o.radius        = s->radius.empty() ? nullptr : s->radius.data();
    o.num_lines     = (int)s->lines.size();
    o.lines         = s->lines.empty() ? nullptr : (const int*)s->lines.data();
    o.num_triangles = s->lines.empty() ? (int)s->triangles.size() : 0;
    o.triangles     = o.num_triangles ? (const int*)s->triangles.data() : nullptr;
    o.texcoords     = s->texcoords.size() == s->positions.size() && !s->texcoords.empty() ? (const float*)s->texcoords.data() : nullptr;
    shapes.push_back(o);
    flat.shape_vertex_edits.push_back(s->vertex_edits);
  }
  for (auto& m : sc->materials) {
    yh_material o{};
    o.emission[0] = m->emission.x, o.emission[1] = m->emission.y, o.emission[2] = m->emission.z;
    o.color[0] = m->color.x, o.color[1] = m->color.y, o.color[2] = m->color.z;
    o.specular = m->specular, o.metallic = m->metallic, o.roughness = m->roughness;
    o.transmission = m->transmission, o.opacity = m->opacity, o.ior = m->ior, o.thin = m->thin;
    o.sigma_a[0] = m->sigma_a.x, o.sigma_a[1] = m->sigma_a.y, o.sigma_a[2] = m->sigma_a.z;
    o.beta_m = m->beta_m, o.beta_n = m->beta_n, o.alpha = m->alpha, o.eta = m->eta;
    o.eumelanin = m->eumelanin, o.pheomelanin = m->pheomelanin;
    o.scattering[0] = m->scattering.x, o.scattering[1] = m->scattering.y, o.scattering[2] = m->scattering.z;
    o.scanisotropy = m->scanisotropy, o.trdepth = m->trdepth;
    o.emission_tex = material_texture(m->emission_tex), o.color_tex = material_texture(m->color_tex);
    o.scattering_tex = material_texture(m->scattering_tex);
    materials.push_back(o);
    yh_material_maps mm{};
    mm.specular_tex = material_texture(m->specular_tex), mm.metallic_tex = material_texture(m->metallic_tex);
    mm.roughness_tex = material_texture(m->roughness_tex), mm.transmission_tex = material_texture(m->transmission_tex);
    mm.opacity_tex = material_texture(m->opacity_tex), mm.normal_tex = material_texture(m->normal_tex);
    maps.push_back(mm);
  }
  for (auto& ob : sc->objects) {
    yh_object o{};
    static_assert(sizeof(frame3f) == 48, "frame3f layout");
    memcpy(o.frame, &ob->frame, 48);
    o.shape = index_of(sc->shapes, ob->shape_), o.material = index_of(sc->materials, ob->material_);
    objects.push_back(o);
  }
  for (auto& e : sc->environments) {
    yh_environment o{};
    memcpy(o.frame, &e->frame, 48);
    o.emission[0] = e->emission.x, o.emission[1] = e->emission.y, o.emission[2] = e->emission.z;
    if (e->emission_tex) {
      o.tex_width = e->emission_tex->width, o.tex_height = e->emission_tex->height;
      o.texels = (const float*)e->emission_tex->colorf.data();
    }
    envs.push_back(o);
  }
  if (!cam) throw std::runtime_error("yhair: no camera");
  auto& c = flat.camera;
  memcpy(c.frame, &cam->frame, 48);
  c.lens = cam->lens, c.film[0] = cam->film.x, c.film[1] = cam->film.y;
  c.focus = cam->focus, c.aperture = cam->aperture;
  return flat;
}
inline void upload_scene(const scene* sc, const camera* cam, detail::flat_scene&& flat) {
  const yh_scene_desc d = flat.desc();
  detail::for_each_context([&](yh_context* ctx, int) { return yh_upload_scene_maps(ctx, &d, flat.maps.data()); });  // the scene is replicated
  sc->uploaded     = std::move(flat);
  sc->uploaded_for = cam;
}
inline void upload_scene(const scene* sc, const camera* cam) { upload_scene(sc, cam, flatten_scene(sc, cam)); }
// Passes the differences classify_edit found on to every context. false: a context refused one (YH_E_INVALID: the contexts that took
// theirs are brought in line by the upload that follows).
inline bool update_scene(const scene* sc, const camera* cam, detail::flat_scene&& flat, unsigned kind) {
  std::atomic<bool> refused{false};  // (every context from a thread of its own)
  detail::for_each_context([&](yh_context* ctx, int) {
    int rc = yh_set_light_edits(ctx, sc->light_edits ? 1 : 0);
    if (!rc && (kind & detail::edit_camera)) rc = yh_update_camera(ctx, &flat.camera);
    if (!rc && (kind & detail::edit_materials)) rc = yh_update_materials(ctx, 0, (int)flat.materials.size(), flat.materials.data());
    if (!rc && (kind & detail::edit_environments)) rc = yh_update_environments(ctx, (int)flat.environments.size(), flat.environments.data());
    if (!rc && (kind & detail::edit_objects)) rc = yh_update_objects(ctx, 0, (int)flat.objects.size(), flat.objects.data());
    if (kind & detail::edit_shapes)
      for (size_t i = 0; i < flat.shapes.size() && !rc; i++)
        if (detail::shape_vertices_differ(sc->uploaded, flat, i)) rc = (sc->shape_refit ? yh_refit_shape : yh_update_shape)(ctx, (int)i, &flat.shapes[i]);
    if (rc == YH_E_INVALID) refused = true, rc = YH_OK;
    return rc;
  });
  if (refused) return false;
  sc->uploaded     = std::move(flat);
  sc->uploaded_for = cam;
  return true;
}
// init_bvh / init_lights: same signatures as pt.h:207-217. They mark the scene;
// the build itself runs inside the upload (see upload_scene).
inline void init_bvh(scene* sc, const trace_params&, progress_callback progress_cb = {}) {
  sc->bvh_requested = true, sc->uploaded_for = nullptr;
  if (progress_cb) progress_cb("build bvh", 1, 1);
}
inline void init_lights(scene* sc, const trace_params&, progress_callback progress_cb = {}) {
  sc->lights_requested = true, sc->uploaded_for = nullptr;
  if (progress_cb) progress_cb("build light", 1, 1);
}
// init_state (pt.cpp:1931-1946)
inline void init_state(state* st, const scene* sc, const camera* cam, const trace_params& params) {
  if ((int)params.shader < 0 || (int)params.shader > (int)shader_type::normal)
    throw std::runtime_error("sampler unknown");  // pt.cpp:1669
  if (!sc->bvh_requested || !sc->lights_requested)
    throw std::runtime_error("yhair: init_state before init_bvh / init_lights");
  // The reference reads its scene structs at every sample, so whatever a caller set since the last init_state is in force from here on
  // (apps/ysceneitraces/ysceneitraces.cpp:392-410: the camera's frame, then reset_display). The contexts hold a flattened copy: compare.
  // Nothing changed: nothing to do. Only what the yh_update_* calls accept (camera fields, material fields, the environments' frames
  // and emission; with set_object_edits, the objects' frames and materials; with set_shape_edits, a shape's vertex arrays — through yh_refit_shape with set_shape_refit): those calls,
  // which keep every shape's tree but an edited shape's own. Anything else
  // — an object's frame without the opt-in, a shape's arrays, a texture, an emission turned on or off (without set_light_edits),
  // init_bvh / init_lights called again — is the whole upload.
  {
    auto     flat = flatten_scene(sc, cam);
    unsigned kind = sc->uploaded_for ? detail::classify_edit(sc->uploaded, flat, sc->object_edits, sc->shape_edits, sc->light_edits) : (unsigned)detail::edit_upload;
    if (kind != detail::edit_none && !(kind & detail::edit_upload)) {
      if (update_scene(sc, cam, std::move(flat), kind)) sc->edits++;
      else kind = detail::edit_upload, flat = flatten_scene(sc, cam);
    }
    if (kind & detail::edit_upload) {
      const auto t0 = std::chrono::steady_clock::now();
      upload_scene(sc, cam, std::move(flat));
      sc->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      sc->uploads++;
    }
  }
  st->device_params = yh_trace_params{params.resolution, params.bounces, params.clamp, params.seed, (int)params.shader, params.hair_exact ? 1 : 0};
  detail::for_each_context([&](yh_context* ctx, int i) {
    int rc = yh_set_shard(ctx, i, (int)detail::contexts().size());
    return rc ? rc : yh_init_state(ctx, &st->device_params);
  });
  detail::check(yh_image_size(detail::require_context(), &st->width, &st->height));
  st->samples = 0;
  st->render.assign((size_t)st->width * st->height, vec4f{});
  detail::bound_state() = st;
}
// The contexts hold the pixels of ONE state. The reference's interactive caller initialises its render state,
// then initialises and traces a low-resolution preview state, then traces the render state
// (apps/ysceneitraces/ysceneitraces.cpp:255-300): a state that was displaced by another init_state before it
// accumulated any sample is simply initialised again on the device; one that had samples cannot be.
inline void bind_state(state* st) {
  if (detail::bound_state() == st) return;
  if (st->samples != 0) throw std::runtime_error("yhair: this state's pixels were displaced by another init_state");
  detail::for_each_context([&](yh_context* ctx, int) { return yh_init_state(ctx, &st->device_params); });
  detail::bound_state() = st;
}
inline void download(state* st) {
  auto& ctxs = detail::require_contexts();
  if (ctxs.size() == 1) detail::check(yh_download(ctxs[0], (float*)st->render.data()));
  else detail::check(yh_gather_framebuffer(ctxs.data(), (int)ctxs.size(), (float*)st->render.data()));
}
// trace_samples (pt.cpp:1992-2007): `nsamples` calls of the reference's
// function in one launch per GPU; state->render is refreshed when `download` is set.
inline void trace_samples(state* st, const scene*, const camera*, const trace_params&, int nsamples = 1,
    bool download_image = true) {
  bind_state(st);
  detail::for_each_context([&](yh_context* ctx, int) { return yh_trace_samples(ctx, nsamples); });
  st->samples += nsamples;
  if (download_image) download(st);
}
// the stop-flag overload (pt.cpp:2009-2026): one sample per call like the reference's; the flag is looked at
// before the launch and again before the image is copied back, so a set flag costs at most one launch.
inline void trace_samples(state* st, const scene* sc, const camera* cam, const trace_params& params,
    std::atomic<bool>* stop) {
  if (stop && *stop) return;
  trace_samples(st, sc, cam, params, 1, false);
  if (stop && *stop) return;
  download(st);
}

// EXTENSION (no reference counterpart): the first-hit feature pass over the image of `st` (include/yhair.h: yh_trace_gbuffer) — per pixel
// what the camera ray meets first and what the `normal` shader evaluates there, for denoising guides, masks and picking. Every plane has
// the state's size, row-major, top row first; misses hold -1 in the id planes and 0 elsewhere. Context 0 alone runs the pass, over the
// whole image however many devices render; the state's samples and `render` are untouched.
template <typename T>
struct image {
  int            width = 0, height = 0;
  std::vector<T> pixels;
  const T& operator[](vec2i ij) const { return pixels[(size_t)ij.y * width + ij.x]; }
};
struct ray6f { vec3f o, d; };
enum struct gbuffer_mode { centre = YH_GBUFFER_CENTRE, next_sample = YH_GBUFFER_NEXT_SAMPLE };
struct gbuffer {
  image<int>   object, element, material;
  image<vec2f> uv;
  image<float> distance;
  image<vec3f> position, normal, tangent;
  image<vec2f> texcoord;
  image<vec3f> albedo;
  image<ray6f> ray;
};
inline gbuffer trace_gbuffer(state* st, const scene*, const camera*, const trace_params&, gbuffer_mode mode = gbuffer_mode::centre) {
  bind_state(st);
  gbuffer g;
  auto    size = [&](auto& im) { im.width = st->width, im.height = st->height, im.pixels.resize((size_t)st->width * st->height); };
  size(g.object), size(g.element), size(g.material), size(g.uv), size(g.distance), size(g.position), size(g.normal), size(g.tangent);
  size(g.texcoord), size(g.albedo), size(g.ray);
  static_assert(sizeof(vec2f) == 8 && sizeof(vec3f) == 12 && sizeof(ray6f) == 24, "the planes are packed floats");
  yh_gbuffer out{g.object.pixels.data(), g.element.pixels.data(), g.material.pixels.data(), (float*)g.uv.pixels.data(),
      g.distance.pixels.data(), (float*)g.position.pixels.data(), (float*)g.normal.pixels.data(), (float*)g.tangent.pixels.data(),
      (float*)g.texcoord.pixels.data(), (float*)g.albedo.pixels.data(), (float*)g.ray.pixels.data()};
  auto ctx = detail::require_context();
  detail::check(yh_trace_gbuffer(ctx, (int)mode, &out), ctx);
  return g;
}

// EXTENSION (no reference counterpart; off unless called): the image of `st` denoised (include/yhair.h: DENOISE) — the edge-avoiding
// a-trous filter guided by the centre-mode feature pass. The image is downloaded first (with several devices: gathered), context 0 alone
// filters it and traces the guides; the state's samples and `render` keep what a download gives them. default_denoise_params: the
// library's defaults for the uploaded scene (call after init_state).
using denoise_params = yh_denoise_params;
inline denoise_params default_denoise_params() {
  denoise_params p;
  detail::check(yh_denoise_default_params(detail::require_context(), &p));
  return p;
}
inline image<vec4f> denoise_image(state* st, const scene*, const camera*, const trace_params&, const denoise_params& dparams) {
  bind_state(st);
  download(st);
  image<vec4f> out;
  out.width = st->width, out.height = st->height, out.pixels.resize((size_t)st->width * st->height);
  auto ctx = detail::require_context();
  detail::check(yh_denoise(ctx, &dparams, (const float*)st->render.data(), (float*)out.pixels.data()), ctx);
  return out;
}

// EXTENSION (no reference counterpart; off unless called): the image of `st` accumulated over the steps of an interactive loop
// (include/yhair.h: TEMPORAL) — the previous call's result reprojected into this view through the centre-mode position plane and blended
// with the state's image by sample count; with `dparams` the accumulated image is then denoised as denoise_image denoises. Context 0
// keeps the history: it survives the camera, object and shape edits init_state passes on and a state of the same size, and starts
// afresh after an upload, a state of another size or a change of the lighting. The state needs at least one sample; its samples and
// `render` keep what a download gives them. default_temporal_params: the library's defaults for the uploaded scene (call after init_state).
using temporal_params = yh_temporal_params;
inline temporal_params default_temporal_params() {
  temporal_params p;
  detail::check(yh_temporal_default_params(detail::require_context(), &p));
  return p;
}
inline image<vec4f> accumulate_image(state* st, const scene*, const camera*, const trace_params&, const temporal_params& tparams,
    const denoise_params* dparams = nullptr) {
  bind_state(st);
  download(st);
  image<vec4f> out;
  out.width = st->width, out.height = st->height, out.pixels.resize((size_t)st->width * st->height);
  auto ctx = detail::require_context();
  detail::check(yh_temporal_accumulate(ctx, &tparams, (const float*)st->render.data(), st->samples, nullptr, (float*)out.pixels.data()), ctx);
  if (dparams) detail::check(yh_denoise(ctx, dparams, (const float*)out.pixels.data(), (float*)out.pixels.data()), ctx);
  return out;
}
// EXTENSION (no reference counterpart; off unless called): accumulate_image with the variance stage (include/yhair.h: VARIANCE) — the state's
// image accumulated with luminance moments beside the colour, the per-pixel variance estimated from them, and the accumulated image through
// the a-trous levels that variance steers. `variance` (optional) receives the filtered variance, one float per pixel. The history is
// accumulate_image's: a call of either advances it, a plain accumulate_image in between starts the moments afresh.
using variance_params = yh_variance_params;
inline variance_params default_variance_params() {
  variance_params p;
  detail::check(yh_variance_default_params(detail::require_context(), &p));
  return p;
}
inline image<vec4f> accumulate_image_variance(state* st, const scene*, const camera*, const trace_params&, const temporal_params& tparams,
    const variance_params& vparams, std::vector<float>* variance = nullptr, bool filtered = true) {
  bind_state(st);
  download(st);
  image<vec4f> out;
  out.width = st->width, out.height = st->height, out.pixels.resize((size_t)st->width * st->height);
  if (variance) variance->resize(out.pixels.size());
  auto   ctx = detail::require_context();
  float* var = variance ? variance->data() : nullptr;
  detail::check(yh_temporal_accumulate_variance(ctx, &tparams, &vparams, (const float*)st->render.data(), st->samples, nullptr, (float*)out.pixels.data(),
                    filtered ? nullptr : var), ctx);
  if (filtered)  // (else: the accumulated image and the variance estimate as they are, for a caller that filters the last step only)
    detail::check(yh_denoise_variance_image(ctx, &vparams, (const float*)out.pixels.data(), nullptr, nullptr, (float*)out.pixels.data(), var), ctx);
  return out;
}
inline void reset_accumulation() { detail::check(yh_temporal_reset(detail::require_context())); }
}  // namespace yhair::pathtrace
#endif
