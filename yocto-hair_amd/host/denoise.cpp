// denoise.cpp — yh_denoise and friends (include/yhair.h: DENOISE): the edge-avoiding a-trous filter over the resolved render, guided by
// the centre-mode planes of the first-hit feature pass (gbuffer.cpp). The arithmetic is unit/atrous_math.h, compiled here for
// yh_atrous_filter (the host's form) and by unit/denoise.hip for the device; this file checks, stages and launches.
#include "image_pass.h"
#include "../unit/atrous_math.h"

namespace {
using yha::V4;
// the form of unit/denoise.hip the context entries run: the faster one by the A/B of tools/denoise_latency.py (profiles/denoise/latency.txt)
constexpr int SHIPPED_FORM = 1;

// The filter's kernels on the context's stream, blocking: d_in (NULL: accum / samples) -> d_out, both float4 device images of w x h
// pixels (they may be the same); g: device planes, only those the parameters read (planes_in). Sets yh_last_trace_ms; `per_kernel`: ctx->dn_ms too.
int run_filter(yh_context* ctx, const char* who, int form, int w, int h, const yh_denoise_params& P, const void* d_in, const yh_gbuffer& g, void* d_out, bool per_kernel) {
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
  if (int rc = timed_begin(ctx)) return rc;
  int e = yhk_dn_pack(d_in, accum, samples, w, h, g.object, g.normal, g.position, g.albedo, N ? u[0].p : d_out, g0.p, g1.p, N == 0, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_dn_pack launch: %s", who, hipGetErrorString((hipError_t)e));
  for (int l = 0; l < N; l++) {
    if (per_kernel) HIPCHK(ctx, hipEventRecord(ev[(size_t)l], ctx->stream));
    const bool last = l == N - 1;
    e = yhk_dn_level(form, w, h, l, &P, u[l & 1].p, g0.p, g1.p, last ? g.albedo : nullptr, last, last ? d_out : u[(l + 1) & 1].p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%s: k_dn_level launch: %s", who, hipGetErrorString((hipError_t)e));
  }
  if (int rc = timed_end(ctx, 1 + N)) return rc;
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
  return state_checks(ctx, who, CHECK_POISONED | NEED_STATE | (own_guides ? NEED_SCENE : 0) | (own_render ? OWN_RENDER : 0));
}

// d_in (NULL: the own render) -> d_out on the device; guides NULL: traced here into temporary planes
int denoise_on_device(yh_context* ctx, const char* who, const yh_denoise_params& P, const void* d_in, const yh_gbuffer* guides, void* d_out) {
  const int w = ctx->state.width, h = ctx->state.height;
  if ((int64_t)w * h > MAX_PIXELS) return refuse_too_many_pixels(ctx, who);
  const unsigned mask = filter_planes(&P);
  Staged         own(ctx);
  yh_gbuffer     g{};
  PassTime       t;
  if (guides) g = planes_in(mask, *guides);
  else if (mask) {
    if (int rc = trace_guides(own, who, mask, g)) return rc;
    t.add(ctx);
  }
  if (int rc = run_filter(ctx, who, SHIPPED_FORM, w, h, P, d_in, g, d_out, false)) return rc;
  t.add(ctx);
  return YH_OK;
}
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

int denoise_with_planes(yh_context* ctx, const char* who, const yh_denoise_params& P, const void* d_in, const yh_gbuffer& guides, void* d_out) {
  return run_filter(ctx, who, SHIPPED_FORM, ctx->state.width, ctx->state.height, P, d_in, planes_in(filter_planes(&P), guides), d_out, false);
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
  if (!aligned16(rgba_in) || !aligned16(rgba_out)) return refuse_unaligned(ctx, who);
  if (guides)
    if (const char* m = missing_plane(filter_planes(p), *guides)) return fail(ctx, YH_E_INVALID, "%s: the parameters need the guide plane `%s`, which is NULL", who, m);
  if (int rc = enter_device(ctx)) return rc;
  return denoise_on_device(ctx, who, *p, rgba_in, guides, rgba_out);
}

int yh_denoise(yh_context* ctx, const yh_denoise_params* p, const float* rgba_in, float* rgba_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise";
  if (int rc = context_checks(ctx, who, p, !rgba_in, true)) return rc;
  if (!rgba_out) return fail(ctx, YH_E_INVALID, "%s: rgba_out is NULL", who);
  if (int rc = enter_device(ctx)) return rc;
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
  if (int rc = enter_device(ctx)) return rc;
  DevBuf img;
  if (int rc = dev_alloc(ctx, img, (size_t)ctx->state.width * ctx->state.height * 16)) return rc;
  if (int rc = ensure_display(ctx, false)) return rc;
  if (int rc = denoise_on_device(ctx, who, *p, nullptr, nullptr, img.p)) return rc;
  PassTime t;
  t.add(ctx);
  return display_tail(ctx, who, img.p, exposure, filmic, srgb, rgba8, t);
}

// ---- the unit-level pair ----------------------------------------------------------------------------------------------------------------
namespace {
bool filter_args(int w, int h, const yh_denoise_params* p, const float* rgba, const yh_gbuffer& g, const float* out) {
  if (w < 1 || h < 1 || (int64_t)w * h > MAX_PIXELS || !p || !yha::params_ok(*p) || !rgba || !out) return false;
  return !missing_plane(filter_planes(p), g);
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
  const yh_gbuffer given = guides_of(object, normal, position, albedo);
  if (!filter_args(w, h, p, rgba, given, out)) return YH_E_INVALID;
  const size_t npix = (size_t)w * h;
  if (p->iterations == 0) {
    if (out != rgba) memmove(out, rgba, npix * 16);
    return YH_OK;
  }
  const yh_gbuffer g = planes_in(filter_planes(p), given);
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
  const yh_gbuffer given = guides_of(object, normal, position, albedo);
  if (!filter_args(w, h, p, rgba, given, out))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, a NULL params, image or output, iterations outside 0 .. %d, or a guide plane the parameters need is NULL", who,
        YH_DENOISE_MAX_ITERATIONS);
  if (int rc = state_checks(ctx, who, CHECK_POISONED)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)w * h;
  Staged       s(ctx);
  void*        img = s.in(rgba, npix * 16);
  yh_gbuffer   dg{};
  for (Plane k : guide_order)
    if (filter_planes(p) & plane_bit(k)) set_plane(dg, k, s.in(plane_of(given, k), plane_bytes[k] * npix));
  if (s.rc) return s.rc;
  if (int rc = run_filter(ctx, who, form, w, h, *p, img, dg, img, true)) return rc;
  HIPCHK(ctx, hipMemcpy(out, img, npix * 16, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_atrous_level_ms(const yh_context* ctx, float* ms, int capacity) {
  if (!ctx) return YH_E_INVALID;
  for (int k = 0; ms && k < std::min(capacity, ctx->dn_ms_count); k++) ms[k] = ctx->dn_ms[k];
  return ctx->dn_ms_count;
}
