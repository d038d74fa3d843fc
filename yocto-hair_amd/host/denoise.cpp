// denoise.cpp — yh_denoise and friends (include/yhair.h: DENOISE): the edge-avoiding a-trous filter over the resolved render, guided by
// the centre-mode planes of the first-hit feature pass (gbuffer.cpp). The arithmetic is unit/atrous_math.h, compiled here for
// yh_atrous_filter (the host's form) and by unit/denoise.hip for the device; this file checks, stages and launches.
#include "context_internal.h"
#include "../unit/atrous_math.h"

namespace {
using yha::V4;

struct Guides {  // the four planes the filter reads; device or host pointers as the caller says
  const int*   object;
  const float *normal, *position, *albedo;
};
// the planes a parameter set reads, the others dropped (so that a plane that is given but not needed changes nothing)
Guides needed_of(const yh_denoise_params& P, Guides g) {
  if (!(P.sigma_normal > 0)) g.normal = nullptr;
  if (!(P.sigma_position > 0)) g.position = nullptr;
  if (!P.demodulate) g.albedo = nullptr;
  return g;
}
const char* missing_plane(const yh_denoise_params& P, const Guides& g) {
  if (!g.object) return "object";
  if (P.sigma_normal > 0 && !g.normal) return "normal";
  if (P.sigma_position > 0 && !g.position) return "position";
  if (P.demodulate && !g.albedo) return "albedo";
  return nullptr;
}
constexpr int64_t MAX_PIXELS = 1ll << 28;
// the form of unit/denoise.hip the context entries run: the faster one by the A/B of tools/denoise_latency.py (profiles/denoise/latency.txt)
constexpr int SHIPPED_FORM = 1;

// The filter's kernels on the context's stream, blocking: d_in (NULL: accum / samples) -> d_out, both float4 device images of w x h
// pixels (they may be the same); g: device planes, already reduced by needed_of. Sets yh_last_trace_ms; `per_kernel`: ctx->dn_ms too.
int run_filter(yh_context* ctx, const char* who, int form, int w, int h, const yh_denoise_params& P, const void* d_in, const Guides& g, void* d_out, bool per_kernel) {
  const size_t npix = (size_t)w * h;
  const int    N    = P.iterations;
  DevBuf       u[2], g0, g1;
  if (N > 0)
    for (DevBuf* b : {&u[0], &u[1], &g0, &g1}) {
      if (b == &u[1] && N < 2) continue;  // (one level goes from u[0] straight to d_out)
      if (int rc = dev_alloc(ctx, *b, npix * 16)) return rc;
    }
  std::vector<hipEvent_t> ev;
  struct EvGuard {
    std::vector<hipEvent_t>& v;
    ~EvGuard() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
  } guard{ev};
  if (per_kernel)
    for (int k = 0; k < N; k++) {
      hipEvent_t e;
      HIPCHK(ctx, hipEventCreate(&e));
      ev.push_back(e);
    }
  const void* accum   = ctx->have_state ? (const void*)ctx->state.accum : nullptr;
  const int   samples = ctx->have_state ? ctx->state.samples_done : 0;
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int e = yhk_dn_pack(d_in, accum, samples, w, h, g.object, g.normal, g.position, g.albedo, N ? u[0].p : d_out, g0.p, g1.p, N == 0, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_dn_pack launch: %s", who, hipGetErrorString((hipError_t)e));
  for (int l = 0; l < N; l++) {
    if (per_kernel) HIPCHK(ctx, hipEventRecord(ev[(size_t)l], ctx->stream));
    const bool last = l == N - 1;
    e = yhk_dn_level(form, w, h, l, &P, u[l & 1].p, g0.p, g1.p, last ? g.albedo : nullptr, last, last ? d_out : u[(l + 1) & 1].p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%s: k_dn_level launch: %s", who, hipGetErrorString((hipError_t)e));
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  YH_WAIT(ctx);
  HIPCHK(ctx, hipEventElapsedTime(&ctx->last_ms, ctx->ev0, ctx->ev1));
  ctx->last_launches = 1 + N;
  if (per_kernel) {
    for (int k = 0; k <= N; k++)
      HIPCHK(ctx, hipEventElapsedTime(&ctx->dn_ms[k], k == 0 ? ctx->ev0 : ev[(size_t)k - 1], k == N ? ctx->ev1 : ev[(size_t)k]));
    ctx->dn_ms_count = 1 + N;
  }
  return YH_OK;
}

// what every context entry refuses, before anything is written
int context_checks(yh_context* ctx, const char* who, const yh_denoise_params* p, bool own_render, bool own_guides) {
  if (!p) return fail(ctx, YH_E_INVALID, "%s: params is NULL", who);
  if (!yha::params_ok(*p)) return fail(ctx, YH_E_INVALID, "%s: %d iterations (0 .. %d)", who, p->iterations, YH_DENOISE_MAX_ITERATIONS);
  if (ctx->poisoned) return refuse_poisoned(ctx);
  if (own_guides && !ctx->have_scene) return fail(ctx, YH_E_STATE, "%s before yh_upload_scene", who);
  if (!ctx->have_state) return fail(ctx, YH_E_STATE, "%s before yh_init_state", who);
  if (ctx->async_pending) return fail(ctx, YH_E_STATE, "%s with an asynchronous launch pending: call yh_synchronize first", who);
  if (own_render && ctx->world > 1)
    return fail(ctx, YH_E_STATE, "%s: rgba_in is NULL on shard %d of %d, which holds part of the image: gather first (yh_gather_framebuffer) and pass the image", who,
        ctx->rank, ctx->world);
  return YH_OK;
}

// d_in (NULL: the own render) -> d_out on the device; guides NULL: traced here into temporary planes
int denoise_on_device(yh_context* ctx, const char* who, const yh_denoise_params& P, const void* d_in, const Guides* guides, void* d_out) {
  const int    w = ctx->state.width, h = ctx->state.height;
  const size_t npix = (size_t)w * h;
  if ((int64_t)npix > MAX_PIXELS) return fail(ctx, YH_E_INVALID, "%s: the image has too many pixels", who);
  if (P.iterations == 0) return run_filter(ctx, who, SHIPPED_FORM, w, h, P, d_in, Guides{}, d_out, false);
  Guides g{};
  DevBuf own[4];
  float  pass_ms = 0;
  if (guides) {
    g = needed_of(P, *guides);
  } else {
    void* planes[11] = {};
    if (int rc = dev_alloc(ctx, own[0], npix * 4)) return rc;
    planes[0] = own[0].p;
    const int   slot[3] = {6, 5, 9};  // yh_gbuffer: normal, position, albedo
    const bool  want[3] = {P.sigma_normal > 0, P.sigma_position > 0, P.demodulate != 0};
    for (int k = 0; k < 3; k++) {
      if (!want[k]) continue;
      if (int rc = dev_alloc(ctx, own[k + 1], npix * 12)) return rc;
      planes[slot[k]] = own[k + 1].p;
    }
    if (int rc = gbuffer_pass(ctx, who, YH_GBUFFER_CENTRE, planes)) return rc;
    pass_ms = ctx->last_ms;
    g = Guides{(const int*)planes[0], (const float*)planes[6], (const float*)planes[5], (const float*)planes[9]};
  }
  if (int rc = run_filter(ctx, who, SHIPPED_FORM, w, h, P, d_in, g, d_out, false)) return rc;
  if (!guides) ctx->last_ms += pass_ms, ctx->last_launches += 1;
  return YH_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

float scene_diagonal(const yh_context* ctx) {  // of the union of the objects' world boxes
  if (!ctx || !ctx->have_scene || ctx->h_obj_boxes.empty()) return 0.0f;
  float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (const yhh::Box& b : ctx->h_obj_boxes)
    for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], b.min[k]), hi[k] = std::max(hi[k], b.max[k]);
  double d2 = 0;
  for (int k = 0; k < 3; k++) d2 += ((double)hi[k] - lo[k]) * ((double)hi[k] - lo[k]);
  return (float)std::sqrt(d2);
}

int denoise_with_planes(yh_context* ctx, const char* who, const yh_denoise_params& P, const void* d_in, const int* object, const float* normal,
    const float* position, const float* albedo, void* d_out) {
  const Guides g = P.iterations > 0 ? needed_of(P, Guides{object, normal, position, albedo}) : Guides{};
  return run_filter(ctx, who, SHIPPED_FORM, ctx->state.width, ctx->state.height, P, d_in, g, d_out, false);
}

int yh_denoise_default_params(const yh_context* ctx, yh_denoise_params* p) {
  if (!p) return YH_E_INVALID;
  *p = yh_denoise_params{5, 4.0f, 0.5f, 0.0f, 1, 1};
  if (ctx && ctx->have_scene && !ctx->h_obj_boxes.empty()) p->sigma_position = 0.05f * scene_diagonal(ctx);
  return YH_OK;
}

int yh_denoise_image_device(yh_context* ctx, const yh_denoise_params* p, const void* rgba_in, const yh_gbuffer* guides, void* rgba_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise_image_device";
  if (int rc = context_checks(ctx, who, p, !rgba_in, !guides)) return rc;
  if (!rgba_out) return fail(ctx, YH_E_INVALID, "%s: rgba_out is NULL", who);
  if (!aligned16(rgba_in) || !aligned16(rgba_out)) return fail(ctx, YH_E_INVALID, "%s: the float4 images must be 16-byte aligned", who);
  Guides g{};
  if (guides) {
    g = Guides{guides->object, guides->normal, guides->position, guides->albedo};
    if (p->iterations > 0)
      if (const char* m = missing_plane(*p, g)) return fail(ctx, YH_E_INVALID, "%s: the parameters need the guide plane `%s`, which is NULL", who, m);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  return denoise_on_device(ctx, who, *p, rgba_in, guides ? &g : nullptr, rgba_out);
}

int yh_denoise(yh_context* ctx, const yh_denoise_params* p, const float* rgba_in, float* rgba_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise";
  if (int rc = context_checks(ctx, who, p, !rgba_in, true)) return rc;
  if (!rgba_out) return fail(ctx, YH_E_INVALID, "%s: rgba_out is NULL", who);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  const size_t bytes = (size_t)ctx->state.width * ctx->state.height * 16;
  DevBuf       img;
  if (int rc = dev_alloc(ctx, img, bytes)) return rc;
  if (rgba_in) HIPCHK(ctx, hipMemcpy(img.p, rgba_in, bytes, hipMemcpyHostToDevice));
  if (int rc = denoise_on_device(ctx, who, *p, rgba_in ? img.p : nullptr, nullptr, img.p)) return rc;
  HIPCHK(ctx, hipMemcpy(rgba_out, img.p, bytes, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_denoise_display(yh_context* ctx, const yh_denoise_params* p, float exposure, int filmic, int srgb, uint8_t* rgba8) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise_display";
  if (int rc = context_checks(ctx, who, p, true, true)) return rc;
  if (!rgba8) return fail(ctx, YH_E_INVALID, "%s: rgba8 is NULL", who);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  const int    w = ctx->state.width, h = ctx->state.height;
  const size_t npix = (size_t)w * h;
  DevBuf       img;
  if (int rc = dev_alloc(ctx, img, npix * 16)) return rc;
  if (!ctx->d_display.p || ctx->d_display.bytes < npix * 4)
    if (int rc = dev_alloc(ctx, ctx->d_display, npix * 4)) return rc;
  if (int rc = denoise_on_device(ctx, who, *p, nullptr, nullptr, img.p)) return rc;
  const float ms       = ctx->last_ms;
  const int   launches = ctx->last_launches;
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int e = yhk_display_image(img.p, w, h, exposure, filmic ? 1 : 0, srgb ? 1 : 0, ctx->d_display.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_display_image launch: %s", who, hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(rgba8, ctx->d_display.p, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  float tm = 0;
  HIPCHK(ctx, hipEventElapsedTime(&tm, ctx->ev0, ctx->ev1));
  ctx->last_ms = ms + tm, ctx->last_launches = launches + 1;
  return YH_OK;
}

// ---- the unit-level pair ----------------------------------------------------------------------------------------------------------------
namespace {
bool filter_args(int w, int h, const yh_denoise_params* p, const float* rgba, const Guides& g, const float* out) {
  if (w < 1 || h < 1 || (int64_t)w * h > MAX_PIXELS || !p || !yha::params_ok(*p) || !rgba || !out) return false;
  return p->iterations == 0 || !missing_plane(*p, g);
}
struct HostFetch {
  const V4 *u, *g0, *g1;
  int       width;
  yha::Tap operator()(int x, int y) const {
    const size_t i = (size_t)y * width + x;
    return yha::Tap{u[i], g0[i], g1[i]};
  }
};
}  // namespace

int yh_atrous_filter(int w, int h, const yh_denoise_params* p, const float* rgba, const int* object, const float* normal, const float* position,
    const float* albedo, float* out) {
  if (!filter_args(w, h, p, rgba, Guides{object, normal, position, albedo}, out)) return YH_E_INVALID;
  const size_t npix = (size_t)w * h;
  if (p->iterations == 0) {
    if (out != rgba) memmove(out, rgba, npix * 16);
    return YH_OK;
  }
  const Guides    g = needed_of(*p, Guides{object, normal, position, albedo});
  std::vector<V4> u[2], g0(npix), g1(npix);
  u[0].resize(npix), u[1].resize(npix);
  for (size_t i = 0; i < npix; i++) {
    const yha::Tap t = yha::pack_pixel(V4{rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]}, i, g.object, g.normal, g.position, g.albedo);
    u[0][i] = t.u, g0[i] = t.g0, g1[i] = t.g1;
  }
  for (int l = 0; l < p->iterations; l++) {
    const HostFetch f{u[l & 1].data(), g0.data(), g1.data(), w};
    V4*             dst = u[(l + 1) & 1].data();
    parallel_for(h, [&](int y) {
      for (int x = 0; x < w; x++) dst[(size_t)y * w + x] = yha::level_pixel(f, x, y, w, h, l, *p);
    });
  }
  const V4* res = u[p->iterations & 1].data();
  for (size_t i = 0; i < npix; i++) {
    const V4 v = yha::remodulate(res[i], i, g.object[i], g.albedo);
    out[4 * i] = v.x, out[4 * i + 1] = v.y, out[4 * i + 2] = v.z, out[4 * i + 3] = v.w;
  }
  return YH_OK;
}

int yh_atrous_filter_gpu(yh_context* ctx, int form, int w, int h, const yh_denoise_params* p, const float* rgba, const int* object, const float* normal,
    const float* position, const float* albedo, float* out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_atrous_filter_gpu";
  if (form != 0 && form != 1) return fail(ctx, YH_E_INVALID, "%s: unknown form %d", who, form);
  if (!filter_args(w, h, p, rgba, Guides{object, normal, position, albedo}, out))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, a NULL params, image or output, iterations outside 0 .. %d, or a guide plane the parameters need is NULL", who,
        YH_DENOISE_MAX_ITERATIONS);
  if (ctx->poisoned) return refuse_poisoned(ctx);
  if (ctx->async_pending) return fail(ctx, YH_E_STATE, "%s with an asynchronous launch pending: call yh_synchronize first", who);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  const size_t npix = (size_t)w * h;
  const Guides hg   = p->iterations ? needed_of(*p, Guides{object, normal, position, albedo}) : Guides{};
  DevBuf       img, d_obj, d_f[3];
  if (int rc = dev_alloc(ctx, img, npix * 16)) return rc;
  HIPCHK(ctx, hipMemcpy(img.p, rgba, npix * 16, hipMemcpyHostToDevice));
  Guides dg{};
  if (hg.object) {
    if (int rc = dev_alloc(ctx, d_obj, npix * 4)) return rc;
    HIPCHK(ctx, hipMemcpy(d_obj.p, hg.object, npix * 4, hipMemcpyHostToDevice));
    dg.object = (const int*)d_obj.p;
  }
  const float*  src[3] = {hg.normal, hg.position, hg.albedo};
  const float** dst[3] = {&dg.normal, &dg.position, &dg.albedo};
  for (int k = 0; k < 3; k++) {
    if (!src[k]) continue;
    if (int rc = dev_alloc(ctx, d_f[k], npix * 12)) return rc;
    HIPCHK(ctx, hipMemcpy(d_f[k].p, src[k], npix * 12, hipMemcpyHostToDevice));
    *dst[k] = (const float*)d_f[k].p;
  }
  if (int rc = run_filter(ctx, who, form, w, h, *p, img.p, dg, img.p, true)) return rc;
  HIPCHK(ctx, hipMemcpy(out, img.p, npix * 16, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_atrous_level_ms(const yh_context* ctx, float* ms, int capacity) {
  if (!ctx) return YH_E_INVALID;
  for (int k = 0; ms && k < std::min(capacity, ctx->dn_ms_count); k++) ms[k] = ctx->dn_ms[k];
  return ctx->dn_ms_count;
}
