// image_pass.cpp — the bodies of image_pass.h: what gbuffer.cpp, denoise.cpp and temporal.cpp share.
#include "image_pass.h"

int state_checks(yh_context* ctx, const char* who, unsigned checks) {
  if ((checks & CHECK_POISONED) && ctx->poisoned) return refuse_poisoned(ctx);
  if ((checks & NEED_SCENE) && !ctx->have_scene) return fail(ctx, YH_E_STATE, "%s before yh_upload_scene", who);
  if ((checks & NEED_STATE) && !ctx->have_state) return fail(ctx, YH_E_STATE, "%s before yh_init_state", who);
  if (ctx->async_pending) return fail(ctx, YH_E_STATE, "%s with an asynchronous launch pending: call yh_synchronize first", who);
  if ((checks & OWN_RENDER) && ctx->world > 1)
    return fail(ctx, YH_E_STATE, "%s: rgba_in is NULL on shard %d of %d, which holds part of the image: gather first (yh_gather_framebuffer) and pass the image", who,
        ctx->rank, ctx->world);
  return YH_OK;
}
int enter_device(yh_context* ctx) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return wait_for_launch(ctx);
}

void* Staged::add(size_t bytes, const void* src, int kind) {
  bufs.emplace_back();
  if (rc == YH_OK) rc = kind == 0 ? upload(ctx, bufs.back(), src, bytes) : kind == 1 ? alloc_zero(ctx, bufs.back(), bytes) : dev_alloc(ctx, bufs.back(), bytes);
  return bufs.back().p;
}

int scratch_guides(Staged& s, unsigned mask, size_t npix, yh_gbuffer& dev) {
  dev = yh_gbuffer{};
  for (Plane k : guide_order)
    if (mask & plane_bit(k)) set_plane(dev, k, s.scratch(plane_bytes[k] * npix));
  return s.rc;
}
int stage_guides(Staged& s, unsigned mask, const yh_gbuffer& host, size_t npix, yh_gbuffer& dev) {
  if (int rc = scratch_guides(s, mask, npix, dev)) return rc;
  for (Plane k : guide_order)
    if (mask & plane_bit(k)) HIPCHK(s.ctx, hipMemcpy(plane_of(dev, k), plane_of(host, k), plane_bytes[k] * npix, hipMemcpyHostToDevice));
  return YH_OK;
}
int trace_guides(Staged& s, const char* who, unsigned mask, yh_gbuffer& dev) {
  if (int rc = scratch_guides(s, mask, (size_t)s.ctx->state.width * s.ctx->state.height, dev)) return rc;
  return gbuffer_pass(s.ctx, who, YH_GBUFFER_CENTRE, dev);
}

int timed_begin(yh_context* ctx) {
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return YH_OK;
}
int timed_stop(yh_context* ctx) {
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  return YH_OK;
}
int timed_read(yh_context* ctx, int launches) {
  YH_WAIT(ctx);
  HIPCHK(ctx, hipEventElapsedTime(&ctx->last_ms, ctx->ev0, ctx->ev1));
  ctx->last_launches = launches;
  return YH_OK;
}
int timed_end(yh_context* ctx, int launches) {
  if (int rc = timed_stop(ctx)) return rc;
  return timed_read(ctx, launches);
}

int ensure_display(yh_context* ctx, bool wait_first) {
  const size_t bytes = (size_t)ctx->state.width * ctx->state.height * 4;
  if (ctx->d_display.p && ctx->d_display.bytes >= bytes) return YH_OK;
  if (wait_first) YH_WAIT(ctx);
  return dev_alloc(ctx, ctx->d_display, bytes);
}
int display_tail(yh_context* ctx, const char* who, const void* d_img, float exposure, int filmic, int srgb, uint8_t* rgba8, PassTime& t) {
  const int w = ctx->state.width, h = ctx->state.height;
  if (int rc = timed_begin(ctx)) return rc;
  int e = yhk_display_image(d_img, w, h, exposure, filmic ? 1 : 0, srgb ? 1 : 0, ctx->d_display.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_display_image launch: %s", who, hipGetErrorString((hipError_t)e));
  if (int rc = timed_stop(ctx)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(rgba8, ctx->d_display.p, (size_t)w * h * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = timed_read(ctx, 1)) return rc;
  t.add(ctx);
  return YH_OK;
}
