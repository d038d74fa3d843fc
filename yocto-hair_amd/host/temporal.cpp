// temporal.cpp — yh_temporal_accumulate and friends (include/yhair.h: TEMPORAL): the previous step's render reprojected into the new view
// through the centre-mode position plane of the first-hit feature pass (gbuffer.cpp), validated and blended by sample count, in front of
// the a-trous filter (denoise.cpp). The arithmetic is unit/reproject_math.h, compiled here for yh_reproject (the host's form) and by
// unit/reproject.hip for the device; this file checks, stages, launches and keeps the history (yh_context::Temporal) between steps.
#include "image_pass.h"
#include "../unit/reproject_math.h"

namespace {
using yht::V4;
static_assert(sizeof(yh_camera) == 17 * 4, "a camera is the 17 floats unit/reproject_math.h reads");
static_assert(sizeof(yhd_object) % 4 == 0 && offsetof(yhd_object, frame) == 0 && offsetof(yhd_object, inv_frame) == 48, "the object rows' frames are read in place");

const float* floats_of(const yh_camera& c) { return c.frame; }  // (frame, lens, film, focus, aperture: contiguous)

// what every context entry refuses, before anything is written
int context_checks(yh_context* ctx, const char* who, const yh_temporal_params* p, bool own_render, int samples_in, const yh_gbuffer* guides,
    unsigned planes = temporal_planes()) {
  if (!p) return fail(ctx, YH_E_INVALID, "%s: params is NULL", who);
  if (!yht::params_ok(*p)) return fail(ctx, YH_E_INVALID, "%s: max_history %d (1 .. 2^30)", who, p->max_history);
  if (!own_render && !yht::samples_ok(samples_in)) return fail(ctx, YH_E_INVALID, "%s: an image with %d samples (1 .. 2^30)", who, samples_in);
  if (guides)
    if (const char* m = missing_plane(planes, *guides)) return fail(ctx, YH_E_INVALID, "%s: the guide plane `%s` is NULL", who, m);
  if (int rc = state_checks(ctx, who, CHECK_POISONED | NEED_SCENE | NEED_STATE | (own_render ? OWN_RENDER : 0))) return rc;
  if (own_render && ctx->state.samples_done < 1) return fail(ctx, YH_E_STATE, "%s: rgba_in is NULL and no sample has been traced", who);
  if (own_render && !yht::samples_ok(ctx->state.samples_done)) return fail(ctx, YH_E_INVALID, "%s: too many samples", who);
  if ((int64_t)ctx->state.width * ctx->state.height > MAX_PIXELS) return refuse_too_many_pixels(ctx, who);
  return YH_OK;
}

// One step on the device, blocking: d_in (NULL: the own render) with `samples` samples and the device planes object / position of `g` ->
// d_out (may be NULL, or d_in) and the other side of the history, which becomes the history. Sets yh_last_trace_ms.
// vp NULL: the plain step, which marks the moment history as none. Else stages M and S of include/yhair.h: VARIANCE — the moment history
// beside the colour's, g.albedo where vp->demodulate is set, the variance into the context's plane and (d_var_out not NULL) a copy there.
int step_on_device(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer& g, void* d_out,
    const yh_variance_params* vp = nullptr, float* d_var_out = nullptr) {
  yh_context::Temporal& T = ctx->tp;
  const int    w = ctx->state.width, h = ctx->state.height, nobj = ctx->scene.num_objects;
  const size_t npix = (size_t)w * h;
  const bool   have = T.have && T.width == w && T.height == h && T.num_objects == nobj;
  const int    from = T.side, to = 1 - T.side;
  for (DevBuf* b : {&T.hc[to], &T.hg[to], &T.hm[to]})
    if (b->bytes < npix * 16 && (vp || b != &T.hm[to]))
      if (int rc = dev_alloc(ctx, *b, npix * 16)) return rc;
  if (vp && T.d_var.bytes < npix * 4)
    if (int rc = dev_alloc(ctx, T.d_var, npix * 4)) return rc;
  if (T.d_frames.bytes < (size_t)nobj * 48)
    if (int rc = dev_alloc(ctx, T.d_frames, (size_t)nobj * 48)) return rc;
  if (T.d_usable.bytes < (size_t)nobj * 4)
    if (int rc = dev_alloc(ctx, T.d_usable, (size_t)nobj * 4)) return rc;
  yht::Motion m{nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (have && nobj > 0) {
    HIPCHK(ctx, hipMemcpyAsync(T.d_usable.p, T.usable.data(), (size_t)nobj * 4, hipMemcpyHostToDevice, ctx->stream));
    const float* rows = (const float*)ctx->d_objects.p;
    m = yht::Motion{rows, rows + 12, (const float*)T.d_frames.p, (const int*)T.d_usable.p, (int)(sizeof(yhd_object) / 4), nobj};
  }
  const yh_camera now = ctx->key_camera;
  if (int rc = timed_begin(ctx)) return rc;
  const int n = d_in ? samples : ctx->state.samples_done;
  int       e;
  if (vp) {
    e = yhk_reproject_m(d_in, ctx->state.accum, n, g.object, g.position, vp->demodulate ? g.albedo : nullptr, w, h, T.hc[from].p, T.hg[from].p,
        have && T.have_moments ? T.hm[from].p : nullptr, have ? 1 : 0, floats_of(now), floats_of(have ? T.camera : now), have && nobj > 0 ? &m : nullptr, &P,
        T.hc[to].p, T.hg[to].p, T.hm[to].p, d_out, ctx->stream);
    if (!e) e = yhk_var_spatial(w, h, &P, vp->min_steps, T.hm[to].p, T.hg[to].p, (float*)T.d_var.p, ctx->stream);
  } else {
    e = yhk_reproject(d_in, ctx->state.accum, n, g.object, g.position, w, h, T.hc[from].p, T.hg[from].p, have ? 1 : 0, floats_of(now),
        floats_of(have ? T.camera : now), have && nobj > 0 ? &m : nullptr, &P, T.hc[to].p, T.hg[to].p, d_out, ctx->stream);
  }
  if (e) return fail(ctx, YH_E_DEVICE, "%s: %s launch: %s", who, vp ? "k_reproject_m / k_var_spatial" : "k_reproject", hipGetErrorString((hipError_t)e));
  if (int rc = timed_stop(ctx)) return rc;
  if (vp && d_var_out) HIPCHK(ctx, hipMemcpyAsync(d_var_out, T.d_var.p, npix * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (nobj > 0)  // the frames this step's history was made under: the rows' own, after the kernel that read the previous ones
    HIPCHK(ctx, hipMemcpy2DAsync(T.d_frames.p, 48, ctx->d_objects.p, sizeof(yhd_object), 48, (size_t)nobj, hipMemcpyDeviceToDevice, ctx->stream));
  T.have = T.have_moments = false;  // (an error below leaves no history)
  if (int rc = timed_read(ctx, vp ? 2 : 1)) return rc;
  T.have = true, T.have_moments = vp != nullptr, T.width = w, T.height = h, T.side = to, T.num_objects = nobj, T.camera = now;
  T.usable.assign((size_t)nobj, 1);
  return YH_OK;
}

// ... with the guides traced here where none are given (guides: DEVICE planes)
int accumulate_on_device(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer* guides, void* d_out,
    const yh_variance_params* vp = nullptr, float* d_var_out = nullptr) {
  if (guides) return step_on_device(ctx, who, P, d_in, samples, *guides, d_out, vp, d_var_out);
  Staged     own(ctx);
  yh_gbuffer g{};
  PassTime   t;
  if (int rc = trace_guides(own, who, moment_planes(vp), g)) return rc;
  t.add(ctx);
  if (int rc = step_on_device(ctx, who, P, d_in, samples, g, d_out, vp, d_var_out)) return rc;
  t.add(ctx);
  return YH_OK;
}
}  // namespace

void temporal_drop(yh_context* ctx) { ctx->tp.have = ctx->tp.have_moments = false; }
void temporal_mark_object(yh_context* ctx, int object) {
  if (ctx->tp.have && object >= 0 && (size_t)object < ctx->tp.usable.size()) ctx->tp.usable[(size_t)object] = 0;
}
// for variance.cpp (image_pass.h): the history is this file's, whichever stage advances it
int temporal_checks(yh_context* ctx, const char* who, const yh_temporal_params* p, bool own_render, int samples_in, const yh_gbuffer* guides, unsigned planes) {
  return context_checks(ctx, who, p, own_render, samples_in, guides, planes);
}
int temporal_step(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer& g, void* d_out,
    const yh_variance_params* vp, float* d_var_out) {
  return step_on_device(ctx, who, P, d_in, samples, g, d_out, vp, d_var_out);
}
int temporal_accumulate(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer* guides, void* d_out,
    const yh_variance_params* vp, float* d_var_out) {
  return accumulate_on_device(ctx, who, P, d_in, samples, guides, d_out, vp, d_var_out);
}

int yh_temporal_default_params(const yh_context* ctx, yh_temporal_params* p) {
  if (!p) return YH_E_INVALID;
  *p = yh_temporal_params{4, 0.2f * scene_diagonal(ctx), 1};
  return YH_OK;
}

int yh_temporal_reset(yh_context* ctx) {
  if (!ctx) return YH_E_INVALID;
  temporal_drop(ctx);
  return YH_OK;
}

int yh_temporal_lengths(yh_context* ctx, int* lengths) {
  if (!ctx) return YH_E_INVALID;
  if (int rc = state_checks(ctx, "yh_temporal_lengths", CHECK_POISONED)) return rc;
  const yh_context::Temporal& T = ctx->tp;
  if (!T.have) return 0;
  const size_t npix = (size_t)T.width * T.height;
  if (!lengths) return (int)npix;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf d_len;
  if (int rc = dev_alloc(ctx, d_len, npix * 4)) return rc;
  int e = yhk_tp_lengths(T.hc[T.side].p, T.width, T.height, (int*)d_len.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "yh_temporal_lengths: k_tp_lengths launch: %s", hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(lengths, d_len.p, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  return (int)npix;
}

int yh_temporal_accumulate_device(yh_context* ctx, const yh_temporal_params* p, const void* rgba_in, int samples_in, const yh_gbuffer* guides, void* rgba_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_temporal_accumulate_device";
  if (int rc = context_checks(ctx, who, p, !rgba_in, samples_in, guides)) return rc;
  if (!aligned16(rgba_in) || !aligned16(rgba_out)) return refuse_unaligned(ctx, who);
  if (int rc = enter_device(ctx)) return rc;
  return accumulate_on_device(ctx, who, *p, rgba_in, samples_in, guides, rgba_out);
}

int yh_temporal_accumulate(yh_context* ctx, const yh_temporal_params* p, const float* rgba_in, int samples_in, const yh_gbuffer* guides, float* rgba_out) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_temporal_accumulate";
  if (int rc = context_checks(ctx, who, p, !rgba_in, samples_in, guides)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)ctx->state.width * ctx->state.height;
  Staged       s(ctx);
  void*        img = rgba_in || rgba_out ? s.scratch(npix * 16) : nullptr;
  if (s.rc) return s.rc;
  if (rgba_in) HIPCHK(ctx, hipMemcpy(img, rgba_in, npix * 16, hipMemcpyHostToDevice));
  yh_gbuffer dg{};
  if (guides)
    if (int rc = stage_guides(s, temporal_planes(), *guides, npix, dg)) return rc;
  if (int rc = accumulate_on_device(ctx, who, *p, rgba_in ? img : nullptr, samples_in, guides ? &dg : nullptr, rgba_out ? img : nullptr)) return rc;
  if (rgba_out) HIPCHK(ctx, hipMemcpy(rgba_out, img, npix * 16, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_temporal_display(yh_context* ctx, const yh_temporal_params* tp, const yh_denoise_params* dp, float exposure, int filmic, int srgb, uint8_t* rgba8) {
  if (!ctx) return YH_E_INVALID;
  const char* who = "yh_temporal_display";
  if (int rc = context_checks(ctx, who, tp, true, 0, nullptr)) return rc;
  if (dp && (dp->iterations < 0 || dp->iterations > YH_DENOISE_MAX_ITERATIONS))
    return fail(ctx, YH_E_INVALID, "%s: %d iterations (0 .. %d)", who, dp->iterations, YH_DENOISE_MAX_ITERATIONS);
  if (!rgba8) return fail(ctx, YH_E_INVALID, "%s: rgba8 is NULL", who);
  if (int rc = enter_device(ctx)) return rc;
  Staged     s(ctx);
  void*      img = s.scratch((size_t)ctx->state.width * ctx->state.height * 16);
  yh_gbuffer g{};
  PassTime   t;
  if (s.rc) return s.rc;
  if (int rc = ensure_display(ctx, false)) return rc;
  if (int rc = trace_guides(s, who, display_planes(dp), g)) return rc;  // one feature pass for both stages
  t.add(ctx);
  if (int rc = step_on_device(ctx, who, *tp, nullptr, 0, g, img)) return rc;
  t.add(ctx);
  if (filter_planes(dp)) {  // (the filter runs)
    if (int rc = denoise_with_planes(ctx, who, *dp, img, g, img)) return rc;
    t.add(ctx);
  }
  return display_tail(ctx, who, img, exposure, filmic, srgb, rgba8, t);
}

// ---- the unit-level pair ----------------------------------------------------------------------------------------------------------------
namespace {
struct UnitArgs {
  int                       w, h;
  const yh_temporal_params* p;
  const float*              rgba;
  int                       samples;
  const int*                object;
  const float *             position, *hist_rgba;
  const int *               hist_length, *hist_object;
  const float*              hist_position;
  const yh_camera *         camera, *prev_camera;
  int                       num_objects;
  const float *             frames, *prev_frames;
  const int*                usable;
  float*                    out_rgba;
  int*                      out_length;
};
bool unit_args_ok(const UnitArgs& a) {
  if (a.w < 1 || a.h < 1 || (int64_t)a.w * a.h > MAX_PIXELS || !a.p || !yht::params_ok(*a.p) || !yht::samples_ok(a.samples)) return false;
  if (!a.rgba || !a.object || !a.position || !a.camera || !a.out_rgba || !a.out_length) return false;
  if (a.hist_length && (!a.hist_rgba || !a.hist_object || !a.hist_position || !a.prev_camera)) return false;
  if (a.frames && (a.num_objects < 0 || !a.prev_frames)) return false;
  return true;
}
// the inverses of `n` frames, as the object rows hold them
std::vector<float> inverses_of(const float* frames, int n) {
  std::vector<float> inv((size_t)n * 12);
  for (int k = 0; k < n; k++) inverse_frame(frames + (size_t)k * 12, true, inv.data() + (size_t)k * 12);
  return inv;
}
// the history as the kernel's two planes
void pack_history(const UnitArgs& a, std::vector<V4>& hc, std::vector<V4>& hg) {
  const size_t npix = (size_t)a.w * a.h;
  hc.resize(npix), hg.resize(npix);
  for (size_t i = 0; i < npix; i++) {
    hc[i] = V4{a.hist_rgba[4 * i], a.hist_rgba[4 * i + 1], a.hist_rgba[4 * i + 2], yht::float_of(a.hist_length[i])};
    hg[i] = V4{a.hist_position[3 * i], a.hist_position[3 * i + 1], a.hist_position[3 * i + 2], yht::float_of(a.hist_object[i])};
  }
}
struct HostHistory {
  const V4 *hc, *hg;
  int       width;
  void operator()(int x, int y, V4& c, V4& g) const {
    const size_t q = (size_t)y * width + x;
    c = hc[q], g = hg[q];
  }
};
}  // namespace

int yh_reproject(int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position, const float* hist_rgba,
    const int* hist_length, const int* hist_object, const float* hist_position, const yh_camera* camera, const yh_camera* prev_camera, int num_objects,
    const float* frames, const float* prev_frames, const int* usable, float* out_rgba, int* out_length) {
  const UnitArgs a{w, h, p, rgba, samples, object, position, hist_rgba, hist_length, hist_object, hist_position, camera, prev_camera, num_objects, frames, prev_frames,
      usable, out_rgba, out_length};
  if (!unit_args_ok(a)) return YH_E_INVALID;
  const bool         have = hist_length != nullptr;
  std::vector<V4>    hc, hg;
  std::vector<float> inv;
  if (have) pack_history(a, hc, hg);
  yht::Motion m{nullptr, nullptr, nullptr, nullptr, 0, 0};
  if (have && frames && num_objects > 0) {
    inv = inverses_of(frames, num_objects);
    m   = yht::Motion{frames, inv.data(), prev_frames, usable, 12, num_objects};
  }
  const float *     cam = floats_of(*camera), *pcam = floats_of(have ? *prev_camera : *camera);
  const bool        same = yht::same_bits(cam, pcam, 17);
  const HostHistory f{hc.data(), hg.data(), w};
  parallel_for(h, [&](int j) {
    for (int i = 0; i < w; i++) {
      const size_t      pix = (size_t)j * w + i;
      const V4          c{rgba[4 * pix], rgba[4 * pix + 1], rgba[4 * pix + 2], rgba[4 * pix + 3]};
      const F3          x{position[3 * pix], position[3 * pix + 1], position[3 * pix + 2]};
      const yht::Result r = yht::reproject_pixel(f, i, j, w, h, c, object[pix], x, samples, cam, pcam, same, m, *p, have);
      out_rgba[4 * pix] = r.out.x, out_rgba[4 * pix + 1] = r.out.y, out_rgba[4 * pix + 2] = r.out.z, out_rgba[4 * pix + 3] = r.out.w;
      out_length[pix] = r.length;
    }
  });
  return YH_OK;
}

int yh_reproject_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position,
    const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position, const yh_camera* camera, const yh_camera* prev_camera,
    int num_objects, const float* frames, const float* prev_frames, const int* usable, float* out_rgba, int* out_length) {
  if (!ctx) return YH_E_INVALID;
  const char*    who = "yh_reproject_gpu";
  const UnitArgs a{w, h, p, rgba, samples, object, position, hist_rgba, hist_length, hist_object, hist_position, camera, prev_camera, num_objects, frames, prev_frames,
      usable, out_rgba, out_length};
  if (!unit_args_ok(a))
    return fail(ctx, YH_E_INVALID, "%s: an empty image, max_history or samples outside 1 .. 2^30, a NULL params, image, plane, camera or output, a history or frames given in part", who);
  if (int rc = state_checks(ctx, who, CHECK_POISONED)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)w * h;
  const bool   have = hist_length != nullptr, moving = have && frames && num_objects > 0;
  Staged       s(ctx);
  void*        img = s.in(rgba, npix * 16);
  yh_gbuffer   g{};
  g.object = (int*)s.in(object, plane_bytes[PLANE_object] * npix), g.position = (float*)s.in(position, plane_bytes[PLANE_position] * npix);
  void *hc[2] = {nullptr, s.scratch(npix * 16)}, *hg[2] = {nullptr, s.scratch(npix * 16)}, *d_len = s.scratch(npix * 4);
  if (have) {
    std::vector<V4> c, hgv;
    pack_history(a, c, hgv);
    hc[0] = s.in(c.data(), npix * 16), hg[0] = s.in(hgv.data(), npix * 16);
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
  int e = yhk_reproject(img, nullptr, samples, g.object, g.position, w, h, hc[0], hg[0], have ? 1 : 0, floats_of(*camera),
      floats_of(have ? *prev_camera : *camera), moving ? &m : nullptr, p, hc[1], hg[1], img, ctx->stream);
  if (!e) e = yhk_tp_lengths(hc[1], w, h, (int*)d_len, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_reproject launch: %s", who, hipGetErrorString((hipError_t)e));
  if (int rc = timed_end(ctx, 2)) return rc;
  HIPCHK(ctx, hipMemcpy(out_rgba, img, npix * 16, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(out_length, d_len, npix * 4, hipMemcpyDeviceToHost));
  return YH_OK;
}
