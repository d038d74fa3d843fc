// variance.cpp — yh_temporal_accumulate_variance, yh_denoise_variance_image and friends (include/yhair.h: VARIANCE): luminance moments carried
// through the temporal stage's reprojection (stage M), a spatial estimate where the moment history is short (stage S), and the a-trous
// levels steered by the variance they filter along (stage F). The arithmetic is unit/variance_math.h, compiled here for the host's forms
// and by unit/variance.hip for the device; this file checks, stages and launches. The history itself is temporal.cpp's (image_pass.h:
// temporal_step): the moment plane lives and dies with the colour's.
#include "image_pass.h"
#include "../unit/variance_math.h"

namespace {
using yht::V4;
// the form of unit/variance.hip's levels the context entries run: the faster one at every level it stages by the A/B of
// tools/variance_latency.py (profiles/variance/latency.txt: x 0.75 - 0.90 of form 0 in the metric's view, x 0.54 - 0.79 where every pixel is
// hit); from level 3 on both forms are one kernel
constexpr int SHIPPED_FORM = 1;

const float* floats_of(const yh_camera& c) { return c.frame; }  // (frame, lens, film, focus, aperture: contiguous)

int params_checks(yh_context* ctx, const char* who, const yh_variance_params* p) {
  if (!p) return fail(ctx, YH_E_INVALID, "%s: the variance params are NULL", who);
  if (p->iterations < 0 || p->iterations > YH_DENOISE_MAX_ITERATIONS)
    return fail(ctx, YH_E_INVALID, "%s: %d iterations (0 .. %d)", who, p->iterations, YH_DENOISE_MAX_ITERATIONS);
  if (p->min_steps < 1) return fail(ctx, YH_E_INVALID, "%s: min_steps %d (>= 1)", who, p->min_steps);
  if (!(p->epsilon > 0)) return fail(ctx, YH_E_INVALID, "%s: epsilon %g (> 0)", who, (double)p->epsilon);
  return YH_OK;
}

// Stage F's kernels on the context's stream, blocking: d_in -> d_out, float4 device images of w x h pixels (they may be the same), d_var ->
// d_var_out (NULL: not written; may be d_var); g: device planes, only those the parameters read. Sets yh_last_trace_ms.
int run_filter(yh_context* ctx, const char* who, int form, int w, int h, const yh_variance_params& P, const void* d_in, const float* d_var, const yh_gbuffer& g,
    void* d_out, float* d_var_out, bool per_kernel = false) {
  const size_t npix = (size_t)w * h;
  const int    N    = P.iterations;
  if (per_kernel) ctx->dn_ms_count = 0;
  if (N == 0) {  // the output is the input
    if (d_out != d_in) HIPCHK(ctx, hipMemcpyAsync(d_out, d_in, npix * 16, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_var_out && d_var_out != d_var) HIPCHK(ctx, hipMemcpyAsync(d_var_out, d_var, npix * 4, hipMemcpyDeviceToDevice, ctx->stream));
    YH_WAIT(ctx);
    ctx->last_ms = 0, ctx->last_launches = 0;
    return YH_OK;
  }
  DevBuf u[2], g0, g1;
  for (DevBuf* b : {&u[0], &u[1], &g0, &g1}) {
    if (b == &u[1] && N < 2) continue;  // (one level goes from u[0] straight to d_out)
    if (int rc = dev_alloc(ctx, *b, npix * 16)) return rc;
  }
  std::vector<hipEvent_t> ev;  // per_kernel: one event in front of every level, as denoise.cpp's run_filter has them
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
  if (int rc = timed_begin(ctx)) return rc;
  int e = yhk_vdn_pack(d_in, nullptr, 0, w, h, d_var, g.object, g.normal, g.position, g.albedo, u[0].p, g0.p, g1.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_vdn_pack launch: %s", who, hipGetErrorString((hipError_t)e));
  for (int l = 0; l < N; l++) {
    if (per_kernel) HIPCHK(ctx, hipEventRecord(ev[(size_t)l], ctx->stream));
    const bool last = l == N - 1;
    e = yhk_vdn_level(form, w, h, l, &P, u[l & 1].p, g0.p, g1.p, last ? g.albedo : nullptr, last, d_in, 1.0f, last ? d_out : u[(l + 1) & 1].p,
        last ? d_var_out : nullptr, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%s: k_vdn_level launch: %s", who, hipGetErrorString((hipError_t)e));
  }
  if (int rc = timed_end(ctx, 1 + N)) return rc;
  if (per_kernel) {  // (yh_atrous_level_ms reports the last unit-level filter call, whichever filter it ran)
    for (int k = 0; k <= N; k++)
      HIPCHK(ctx, hipEventElapsedTime(&ctx->dn_ms[k], k == 0 ? ctx->ev0 : ev[(size_t)k - 1], k == N ? ctx->ev1 : ev[(size_t)k]));
    ctx->dn_ms_count = 1 + N;
  }
  return YH_OK;
}

// what the stage-F context entries refuse, before anything is written
int filter_checks(yh_context* ctx, const char* who, const yh_variance_params* p, const void* rgba_in, const float* variance_in, const yh_gbuffer* guides,
    const void* rgba_out) {
  if (int rc = params_checks(ctx, who, p)) return rc;
  if (!rgba_in || !rgba_out) return fail(ctx, YH_E_INVALID, "%s: rgba_in or rgba_out is NULL", who);
  if (guides)
    if (const char* m = missing_plane(variance_filter_planes(p), *guides))
      return fail(ctx, YH_E_INVALID, "%s: the parameters need the guide plane `%s`, which is NULL", who, m);
  if (int rc = state_checks(ctx, who, CHECK_POISONED | NEED_STATE | (guides ? 0 : NEED_SCENE))) return rc;
  if ((int64_t)ctx->state.width * ctx->state.height > MAX_PIXELS) return refuse_too_many_pixels(ctx, who);
  const yh_context::Temporal& T = ctx->tp;
  if (!variance_in && !(T.have && T.have_moments && T.width == ctx->state.width && T.height == ctx->state.height))
    return fail(ctx, YH_E_STATE, "%s: variance_in is NULL and the context keeps no variance of this image: call yh_temporal_accumulate_variance first", who);
  return YH_OK;
}

// d_in -> d_out on the device; guides NULL: traced here into temporary planes; d_var NULL: the context's own
int filter_on_device(yh_context* ctx, const char* who, const yh_variance_params& P, const void* d_in, const float* d_var, const yh_gbuffer* guides, void* d_out,
    float* d_var_out) {
  const unsigned mask = variance_filter_planes(&P);
  Staged         own(ctx);
  yh_gbuffer     g{};
  PassTime       t;
  if (guides) g = planes_in(mask, *guides);
  else if (mask) {
    if (int rc = trace_guides(own, who, mask, g)) return rc;
    t.add(ctx);
  }
  if (int rc = run_filter(ctx, who, SHIPPED_FORM, ctx->state.width, ctx->state.height, P, d_in, d_var ? d_var : (const float*)ctx->tp.d_var.p, g, d_out, d_var_out))
    return rc;
  t.add(ctx);
  return YH_OK;
}
}  // namespace

int yh_variance_default_params(const yh_context* ctx, yh_variance_params* p) {
  if (!p) return YH_E_INVALID;
  yh_denoise_params d;
  if (int rc = yh_denoise_default_params(ctx, &d)) return rc;
  *p = yh_variance_params{4, 2.0f, d.sigma_normal, d.sigma_position, d.demodulate, d.match_object, 1e-2f, 4};  // (profiles/variance/quality.txt)
  return YH_OK;
}

int yh_temporal_accumulate_variance_device(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, const void* rgba_in, int samples_in,
    const yh_gbuffer* guides, void* rgba_out, float* variance_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_temporal_accumulate_variance_device";
  if (int rc = params_checks(ctx, who, vp)) return rc;
  if (int rc = temporal_checks(ctx, who, tp, !rgba_in, samples_in, guides, moment_planes(vp))) return rc;
  if (!aligned16(rgba_in) || !aligned16(rgba_out)) return refuse_unaligned(ctx, who);
  if (int rc = enter_device(ctx)) return rc;
  return temporal_accumulate(ctx, who, *tp, rgba_in, samples_in, guides, rgba_out, vp, variance_out);
}

int yh_temporal_accumulate_variance(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, const float* rgba_in, int samples_in,
    const yh_gbuffer* guides, float* rgba_out, float* variance_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_temporal_accumulate_variance";
  if (int rc = params_checks(ctx, who, vp)) return rc;
  if (int rc = temporal_checks(ctx, who, tp, !rgba_in, samples_in, guides, moment_planes(vp))) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)ctx->state.width * ctx->state.height;
  Staged       s(ctx);
  void*        img = rgba_in || rgba_out ? s.scratch(npix * 16) : nullptr;
  float*       var = variance_out ? (float*)s.scratch(npix * 4) : nullptr;
  if (s.rc) return s.rc;
  if (rgba_in) HIPCHK(ctx, hipMemcpy(img, rgba_in, npix * 16, hipMemcpyHostToDevice));
  yh_gbuffer dg{};
  if (guides)
    if (int rc = stage_guides(s, moment_planes(vp), *guides, npix, dg)) return rc;
  if (int rc = temporal_accumulate(ctx, who, *tp, rgba_in ? img : nullptr, samples_in, guides ? &dg : nullptr, rgba_out ? img : nullptr, vp, var)) return rc;
  if (rgba_out) HIPCHK(ctx, hipMemcpy(rgba_out, img, npix * 16, hipMemcpyDeviceToHost));
  if (variance_out) HIPCHK(ctx, hipMemcpy(variance_out, var, npix * 4, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_denoise_variance_image_device(yh_context* ctx, const yh_variance_params* vp, const void* rgba_in, const float* variance_in, const yh_gbuffer* guides,
    void* rgba_out, float* variance_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise_variance_image_device";
  if (int rc = filter_checks(ctx, who, vp, rgba_in, variance_in, guides, rgba_out)) return rc;
  if (!aligned16(rgba_in) || !aligned16(rgba_out)) return refuse_unaligned(ctx, who);
  if (int rc = enter_device(ctx)) return rc;
  return filter_on_device(ctx, who, *vp, rgba_in, variance_in, guides, rgba_out, variance_out);
}

int yh_denoise_variance_image(yh_context* ctx, const yh_variance_params* vp, const float* rgba_in, const float* variance_in, const yh_gbuffer* guides,
    float* rgba_out, float* variance_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_denoise_variance_image";
  if (int rc = filter_checks(ctx, who, vp, rgba_in, variance_in, guides, rgba_out)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)ctx->state.width * ctx->state.height;
  Staged       s(ctx);
  void*        img = s.in(rgba_in, npix * 16);
  float*       var = variance_in ? (float*)s.in(variance_in, npix * 4) : variance_out ? (float*)s.scratch(npix * 4) : nullptr;
  if (s.rc) return s.rc;
  yh_gbuffer dg{};
  if (guides)
    if (int rc = stage_guides(s, variance_filter_planes(vp), *guides, npix, dg)) return rc;
  if (int rc = filter_on_device(ctx, who, *vp, img, variance_in ? var : nullptr, guides ? &dg : nullptr, img, variance_out ? var : nullptr)) return rc;
  HIPCHK(ctx, hipMemcpy(rgba_out, img, npix * 16, hipMemcpyDeviceToHost));
  if (variance_out) HIPCHK(ctx, hipMemcpy(variance_out, var, npix * 4, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_svgf_display(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, float exposure, int filmic, int srgb, uint8_t* rgba8) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_svgf_display";
  if (int rc = params_checks(ctx, who, vp)) return rc;
  if (int rc = temporal_checks(ctx, who, tp, true, 0, nullptr, 0)) return rc;
  if (!rgba8) return fail(ctx, YH_E_INVALID, "%s: rgba8 is NULL", who);
  if (int rc = enter_device(ctx)) return rc;
  Staged     s(ctx);
  void*      img = s.scratch((size_t)ctx->state.width * ctx->state.height * 16);
  yh_gbuffer g{};
  PassTime   t;
  if (s.rc) return s.rc;
  if (int rc = ensure_display(ctx, false)) return rc;
  if (int rc = trace_guides(s, who, svgf_planes(vp), g)) return rc;  // one feature pass for every stage
  t.add(ctx);
  if (int rc = temporal_step(ctx, who, *tp, nullptr, 0, g, img, vp, nullptr)) return rc;
  t.add(ctx);
  if (int rc = run_filter(ctx, who, SHIPPED_FORM, ctx->state.width, ctx->state.height, *vp, img, (const float*)ctx->tp.d_var.p,
          planes_in(variance_filter_planes(vp), g), img, nullptr))
    return rc;
  t.add(ctx);
  return display_tail(ctx, who, img, exposure, filmic, srgb, rgba8, t);
}

int yh_temporal_steps(yh_context* ctx, int* steps) {
  if (!ctx) return YH_E_INVALID;
  if (int rc = state_checks(ctx, "yh_temporal_steps", CHECK_POISONED)) return rc;
  const yh_context::Temporal& T = ctx->tp;
  if (!T.have || !T.have_moments) return 0;
  const size_t npix = (size_t)T.width * T.height;
  if (!steps) return (int)npix;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf d_steps;
  if (int rc = dev_alloc(ctx, d_steps, npix * 4)) return rc;
  int e = yhk_var_steps(T.hm[T.side].p, T.width, T.height, (int*)d_steps.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "yh_temporal_steps: k_var_steps launch: %s", hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(steps, d_steps.p, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  return (int)npix;
}

// ---- the unit-level pairs ---------------------------------------------------------------------------------------------------------------
namespace {
struct MomentArgs {
  int                       w, h;
  const yh_temporal_params* p;
  const float*              rgba;
  int                       samples;
  const int*                object;
  const float *             position, *albedo, *hist_rgba;
  const int *               hist_length, *hist_object;
  const float *             hist_position, *hist_moments;
  const int*                hist_steps;
  const yh_camera *         camera, *prev_camera;
  int                       num_objects;
  const float *             frames, *prev_frames;
  const int*                usable;
  float*                    out_rgba;
  int*                      out_length;
  float*                    out_moments;
  int*                      out_steps;
};
bool moment_args_ok(const MomentArgs& a) {
  if (a.w < 1 || a.h < 1 || (int64_t)a.w * a.h > MAX_PIXELS || !a.p || !yht::params_ok(*a.p) || !yht::samples_ok(a.samples)) return false;
  if (!a.rgba || !a.object || !a.position || !a.camera || !a.out_rgba || !a.out_length || !a.out_moments || !a.out_steps) return false;
  if (a.hist_length && (!a.hist_rgba || !a.hist_object || !a.hist_position || !a.prev_camera)) return false;
  if ((a.hist_moments == nullptr) != (a.hist_steps == nullptr)) return false;
  if (a.frames && (a.num_objects < 0 || !a.prev_frames)) return false;
  return true;
}
std::vector<float> inverses_of(const float* frames, int n) {
  std::vector<float> inv((size_t)n * 12);
  for (int k = 0; k < n; k++) inverse_frame(frames + (size_t)k * 12, true, inv.data() + (size_t)k * 12);
  return inv;
}
// the history as the kernel's three planes (hm empty: no moment history)
void pack_history(const MomentArgs& a, std::vector<V4>& hc, std::vector<V4>& hg, std::vector<V4>& hm) {
  const size_t npix = (size_t)a.w * a.h;
  hc.resize(npix), hg.resize(npix);
  if (a.hist_moments) hm.resize(npix);
  for (size_t i = 0; i < npix; i++) {
    hc[i] = V4{a.hist_rgba[4 * i], a.hist_rgba[4 * i + 1], a.hist_rgba[4 * i + 2], yht::float_of(a.hist_length[i])};
    hg[i] = V4{a.hist_position[3 * i], a.hist_position[3 * i + 1], a.hist_position[3 * i + 2], yht::float_of(a.hist_object[i])};
    if (a.hist_moments) hm[i] = yhv::plane_of(yhv::Moments{a.hist_moments[2 * i], a.hist_moments[2 * i + 1], a.hist_steps[i]});
  }
}
// stage M's outputs as stage S's two planes
void pack_moments(size_t npix, const float* moments, const int* steps, const int* object, const float* position, std::vector<V4>& hm, std::vector<V4>& hg) {
  hm.resize(npix), hg.resize(npix);
  for (size_t i = 0; i < npix; i++) {
    hm[i] = yhv::plane_of(yhv::Moments{moments[2 * i], moments[2 * i + 1], steps[i]});
    hg[i] = V4{position[3 * i], position[3 * i + 1], position[3 * i + 2], yht::float_of(object[i])};
  }
}
bool spatial_args_ok(int w, int h, const yh_temporal_params* tp, int min_steps, const float* moments, const int* steps, const int* object, const float* position,
    const float* out) {
  return w >= 1 && h >= 1 && (int64_t)w * h <= MAX_PIXELS && tp && min_steps >= 1 && moments && steps && object && position && out;
}
bool filter_args(int w, int h, const yh_variance_params* p, const float* rgba, const float* variance, const yh_gbuffer& g, const float* out) {
  if (w < 1 || h < 1 || (int64_t)w * h > MAX_PIXELS || !p || !yhv::params_ok(*p) || !rgba || !variance || !out) return false;
  return !missing_plane(variance_filter_planes(p), g);
}
struct HostFetch {
  const yha::V4 *u, *g0, *g1;
  int            width;
  yha::Tap operator()(int x, int y) const {
    const size_t i = (size_t)y * width + x;
    return yha::Tap{u[i], g0[i], g1[i]};
  }
};
}  // namespace

int yh_reproject_moments(int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position, const float* albedo,
    const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position, const float* hist_moments, const int* hist_steps,
    const yh_camera* camera, const yh_camera* prev_camera, int num_objects, const float* frames, const float* prev_frames, const int* usable, float* out_rgba,
    int* out_length, float* out_moments, int* out_steps) {
  const MomentArgs a{w, h, p, rgba, samples, object, position, albedo, hist_rgba, hist_length, hist_object, hist_position, hist_moments, hist_steps, camera,
      prev_camera, num_objects, frames, prev_frames, usable, out_rgba, out_length, out_moments, out_steps};
  if (!moment_args_ok(a)) return YH_E_INVALID;
  const bool         have = hist_length != nullptr;
  std::vector<V4>    hc, hg, hm;
  std::vector<float> inv;
  if (have) pack_history(a, hc, hg, hm);
  yht::Motion m{nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (have && frames && num_objects > 0) {
    inv = inverses_of(frames, num_objects);
    m   = yht::Motion{frames, inv.data(), prev_frames, usable, 12, num_objects};
  }
  const float *cam = floats_of(*camera), *pcam = floats_of(have ? *prev_camera : *camera);
  const bool   same = yht::same_bits(cam, pcam, 17);
  const V4 *   pc = hc.data(), *pg = hg.data(), *pm = hm.empty() ? nullptr : hm.data();
  const auto   f = [&](int x, int y, V4& c, V4& g, V4& mo) {
    const size_t q = (size_t)y * w + x;
    c = pc[q], g = pg[q];
    mo = pm ? pm[q] : V4{0.0f, 0.0f, 0.0f, 0.0f};
  };
  parallel_for(h, [&](int j) {
    for (int i = 0; i < w; i++) {
      const size_t pix = (size_t)j * w + i;
      const V4     c{rgba[4 * pix], rgba[4 * pix + 1], rgba[4 * pix + 2], rgba[4 * pix + 3]};
      const F3     x{position[3 * pix], position[3 * pix + 1], position[3 * pix + 2]};
      float        eff[3];
      yha::pixel_albedo(albedo, pix, object[pix], eff);
      const yhv::ResultM r = yhv::reproject_pixel_m(f, i, j, w, h, c, eff, object[pix], x, samples, cam, pcam, same, m, *p, have);
      out_rgba[4 * pix] = r.out.x, out_rgba[4 * pix + 1] = r.out.y, out_rgba[4 * pix + 2] = r.out.z, out_rgba[4 * pix + 3] = r.out.w;
      out_length[pix] = r.length;
      out_moments[2 * pix] = r.m.m1, out_moments[2 * pix + 1] = r.m.m2, out_steps[pix] = r.m.steps;
    }
  });
  return YH_OK;
}

int yh_reproject_moments_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position,
    const float* albedo, const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position, const float* hist_moments,
    const int* hist_steps, const yh_camera* camera, const yh_camera* prev_camera, int num_objects, const float* frames, const float* prev_frames, const int* usable,
    float* out_rgba, int* out_length, float* out_moments, int* out_steps) {
  if (!ctx) return YH_E_INVALID;
  const char*      who = "yh_reproject_moments_gpu";
  const MomentArgs a{w, h, p, rgba, samples, object, position, albedo, hist_rgba, hist_length, hist_object, hist_position, hist_moments, hist_steps, camera,
      prev_camera, num_objects, frames, prev_frames, usable, out_rgba, out_length, out_moments, out_steps};
  if (!moment_args_ok(a))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, max_history or samples outside 1 .. 2^30, a NULL params, image, plane, camera or output, a history, a moment history or frames given in part", who);
  if (int rc = state_checks(ctx, who, CHECK_POISONED)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)w * h;
  const bool   have = hist_length != nullptr, moving = have && frames && num_objects > 0;
  Staged       s(ctx);
  void*        img   = s.in(rgba, npix * 16);
  const int*   d_obj = (const int*)s.in(object, plane_bytes[PLANE_object] * npix);
  const float *d_pos = (const float*)s.in(position, plane_bytes[PLANE_position] * npix),
              *d_alb = albedo ? (const float*)s.in(albedo, plane_bytes[PLANE_albedo] * npix) : nullptr;
  void *hc[2] = {nullptr, s.scratch(npix * 16)}, *hg[2] = {nullptr, s.scratch(npix * 16)}, *hm[2] = {nullptr, s.scratch(npix * 16)};
  if (have) {
    std::vector<V4> c, g, mo;
    pack_history(a, c, g, mo);
    hc[0] = s.in(c.data(), npix * 16), hg[0] = s.in(g.data(), npix * 16);
    if (!mo.empty()) hm[0] = s.in(mo.data(), npix * 16);
  }
  yht::Motion m{nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (moving) {
    const std::vector<float> inv   = inverses_of(frames, num_objects);
    const size_t             bytes = (size_t)num_objects * 48;
    const float *            d_fr = (const float*)s.in(frames, bytes), *d_inv = (const float*)s.in(inv.data(), bytes), *d_prev = (const float*)s.in(prev_frames, bytes);
    m = yht::Motion{d_fr, d_inv, d_prev, usable ? (const int*)s.in(usable, (size_t)num_objects * 4) : nullptr, 12, num_objects};
  }
  if (s.rc) return s.rc;
  if (int rc = timed_begin(ctx)) return rc;
  int e = yhk_reproject_m(img, nullptr, samples, d_obj, d_pos, d_alb, w, h, hc[0], hg[0], hm[0], have ? 1 : 0, floats_of(*camera),
      floats_of(have ? *prev_camera : *camera), moving ? &m : nullptr, p, hc[1], hg[1], hm[1], img, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_reproject_m launch: %s", who, hipGetErrorString((hipError_t)e));
  if (int rc = timed_end(ctx, 1)) return rc;
  std::vector<V4> c(npix), mo(npix);
  HIPCHK(ctx, hipMemcpy(out_rgba, img, npix * 16, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(c.data(), hc[1], npix * 16, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(mo.data(), hm[1], npix * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < npix; i++)
    out_length[i] = yht::bits_of(c[i].w), out_moments[2 * i] = mo[i].x, out_moments[2 * i + 1] = mo[i].y, out_steps[i] = yht::bits_of(mo[i].z);
  return YH_OK;
}

int yh_variance_spatial(int w, int h, const yh_temporal_params* tp, int min_steps, const float* moments, const int* steps, const int* object,
    const float* position, float* out_variance) {
  if (!spatial_args_ok(w, h, tp, min_steps, moments, steps, object, position, out_variance)) return YH_E_INVALID;
  std::vector<V4> hm, hg;
  pack_moments((size_t)w * h, moments, steps, object, position, hm, hg);
  const V4 * pm = hm.data(), *pg = hg.data();
  const auto f  = [&](int x, int y, V4& m, V4& g) {
    const size_t q = (size_t)y * w + x;
    m = pm[q], g = pg[q];
  };
  parallel_for(h, [&](int y) {
    for (int x = 0; x < w; x++) out_variance[(size_t)y * w + x] = yhv::spatial_pixel(f, x, y, w, h, *tp, min_steps);
  });
  return YH_OK;
}

int yh_variance_spatial_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* tp, int min_steps, const float* moments, const int* steps, const int* object,
    const float* position, float* out_variance) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_variance_spatial_gpu";
  if (!spatial_args_ok(w, h, tp, min_steps, moments, steps, object, position, out_variance))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, min_steps < 1, or a NULL params, plane or output", who);
  if (int rc = state_checks(ctx, who, CHECK_POISONED)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t    npix = (size_t)w * h;
  std::vector<V4> hm, hg;
  pack_moments(npix, moments, steps, object, position, hm, hg);
  Staged s(ctx);
  void * d_hm = s.in(hm.data(), npix * 16), *d_hg = s.in(hg.data(), npix * 16), *d_var = s.scratch(npix * 4);
  if (s.rc) return s.rc;
  if (int rc = timed_begin(ctx)) return rc;
  int e = yhk_var_spatial(w, h, tp, min_steps, d_hm, d_hg, (float*)d_var, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_var_spatial launch: %s", who, hipGetErrorString((hipError_t)e));
  if (int rc = timed_end(ctx, 1)) return rc;
  HIPCHK(ctx, hipMemcpy(out_variance, d_var, npix * 4, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_atrous_variance_filter(int w, int h, const yh_variance_params* p, const float* rgba, const float* variance, const int* object, const float* normal,
    const float* position, const float* albedo, float* out, float* out_variance) {
  const yh_gbuffer given = guides_of(object, normal, position, albedo);
  if (!filter_args(w, h, p, rgba, variance, given, out)) return YH_E_INVALID;
  const size_t npix = (size_t)w * h;
  if (p->iterations == 0) {
    if (out != rgba) memmove(out, rgba, npix * 16);
    if (out_variance && out_variance != variance) memmove(out_variance, variance, npix * 4);
    return YH_OK;
  }
  const yh_gbuffer     g = planes_in(variance_filter_planes(p), given);
  std::vector<yha::V4> u[2], g0(npix), g1(npix);
  u[0].resize(npix), u[1].resize(npix);
  for (size_t i = 0; i < npix; i++) {
    const yha::Tap t = yhv::pack_pixel(yha::V4{rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]}, variance[i], i, g.object, g.normal, g.position, g.albedo);
    u[0][i] = t.u, g0[i] = t.g0, g1[i] = t.g1;
  }
  for (int l = 0; l < p->iterations; l++) {
    const HostFetch f{u[l & 1].data(), g0.data(), g1.data(), w};
    yha::V4*        dst = u[(l + 1) & 1].data();
    parallel_for(h, [&](int y) {
      for (int x = 0; x < w; x++) dst[(size_t)y * w + x] = yhv::level_pixel(f, x, y, w, h, l, *p);
    });
  }
  const yha::V4* res = u[p->iterations & 1].data();
  for (size_t i = 0; i < npix; i++) {
    const yha::V4 v     = yha::remodulate(res[i], i, g.object[i], g.albedo);
    const float   alpha = rgba[4 * i + 3] / 1.0f;  // (read before the store: out may be rgba)
    if (out_variance) out_variance[i] = res[i].w;
    out[4 * i] = v.x, out[4 * i + 1] = v.y, out[4 * i + 2] = v.z, out[4 * i + 3] = alpha;
  }
  return YH_OK;
}

int yh_atrous_variance_filter_gpu(yh_context* ctx, int form, int w, int h, const yh_variance_params* p, const float* rgba, const float* variance, const int* object,
    const float* normal, const float* position, const float* albedo, float* out, float* out_variance) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_atrous_variance_filter_gpu";
  if (form != 0 && form != 1) return fail(ctx, YH_E_INVALID, "%s: unknown form %d", who, form);
  const yh_gbuffer given = guides_of(object, normal, position, albedo);
  if (!filter_args(w, h, p, rgba, variance, given, out))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, a NULL params, image, variance or output, iterations outside 0 .. %d, min_steps < 1, epsilon not > 0, or a guide plane the parameters need is NULL",
        who, YH_DENOISE_MAX_ITERATIONS);
  if (int rc = state_checks(ctx, who, CHECK_POISONED)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)w * h;
  Staged       s(ctx);
  void*        img = s.in(rgba, npix * 16);
  float*       var = (float*)s.in(variance, npix * 4);
  yh_gbuffer   dg{};
  for (Plane k : guide_order)
    if (variance_filter_planes(p) & plane_bit(k)) set_plane(dg, k, s.in(plane_of(given, k), plane_bytes[k] * npix));
  if (s.rc) return s.rc;
  if (int rc = run_filter(ctx, who, form, w, h, *p, img, var, dg, img, var, true)) return rc;
  HIPCHK(ctx, hipMemcpy(out, img, npix * 16, hipMemcpyDeviceToHost));
  if (out_variance) HIPCHK(ctx, hipMemcpy(out_variance, var, npix * 4, hipMemcpyDeviceToHost));
  return YH_OK;
}
