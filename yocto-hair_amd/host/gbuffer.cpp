// gbuffer.cpp — yh_trace_gbuffer / yh_trace_gbuffer_device: the first-hit feature pass (unit/gbuffer.hip) over the image of yh_init_state.
#include "context_internal.h"

extern "C" {
int yhk_gbuffer_waves(void);
int yhk_gbuffer_occupancy(const yhd_scene* sc);
int yhk_gbuffer(const yhd_scene* sc, const yhd_scene* sc_dev, const yhd_state* st, int mode, void* const planes[11], int* cursor,
    unsigned int* stack_ovf, int ovf_entries, int grid_blocks, hipStream_t stream);
}

namespace {
constexpr int PLANES = 11;
// bytes per pixel of the planes of yh_gbuffer, in its order
constexpr size_t plane_bytes[PLANES] = {4, 4, 4, 8, 4, 12, 12, 12, 8, 12, 24};
static_assert(sizeof(yh_gbuffer) == PLANES * sizeof(void*), "yh_gbuffer is eleven pointers");

// The pass into `planes` (device pointers, NULL = skipped). Reads the render state, writes none of it.
int gbuffer_impl(yh_context* ctx, const char* who, int mode, void* const planes[PLANES]) {
  const int64_t npix  = (int64_t)ctx->state.width * ctx->state.height;
  const int64_t items = (int64_t)ctx->state.tiles_x * tiles_of(ctx->state.height) * 64;  // the cursor's range: whole 8x8 tiles
  if (items > (1ll << 30)) return fail(ctx, YH_E_INVALID, "%s: the image has too many pixels for the pass's 32-bit cursor", who);
  const int occupancy = std::min(yhk_gbuffer_waves(), yhk_gbuffer_occupancy(&ctx->scene));  // (256-thread blocks: one wave per SIMD each)
  if (occupancy < 1) return fail(ctx, YH_E_DEVICE, "%s: k_gbuffer cannot run with its LDS layout on this device", who);
  const int grid        = (int)std::max<int64_t>(1, std::min<int64_t>((npix + 255) / 256, (int64_t)ctx->num_cus * occupancy));
  const int ovf_entries = 2 * std::max(8, ctx->stack_need);  // (as yh_intersect_batch sizes it)
  DevBuf    cursor, ovf;
  int       rc;
  if ((rc = alloc_zero(ctx, cursor, 16)) || (rc = alloc_zero(ctx, ovf, (size_t)grid * 4 * ovf_entries * 64 * 4))) return rc;
  if (!ctx->d_scene_copy.p && (rc = upload(ctx, ctx->d_scene_copy, &ctx->scene, sizeof(yhd_scene)))) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int e = yhk_gbuffer(&ctx->scene, (const yhd_scene*)ctx->d_scene_copy.p, &ctx->state, mode, planes, (int*)cursor.p, (unsigned int*)ovf.p, ovf_entries, grid, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_gbuffer launch: %s", who, hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  YH_WAIT(ctx);
  HIPCHK(ctx, hipEventElapsedTime(&ctx->last_ms, ctx->ev0, ctx->ev1));  // (yh_last_trace_ms: the kernel alone, without the copies)
  ctx->last_launches = 1;
  return YH_OK;
}

int gbuffer_checks(yh_context* ctx, const char* who, int mode, const yh_gbuffer* out, void* planes[PLANES]) {
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "%s before yh_upload_scene", who);
  if (!ctx->have_state) return fail(ctx, YH_E_STATE, "%s before yh_init_state", who);
  if (ctx->async_pending) return fail(ctx, YH_E_STATE, "%s with an asynchronous launch pending: call yh_synchronize first", who);
  if (mode != YH_GBUFFER_CENTRE && mode != YH_GBUFFER_NEXT_SAMPLE) return fail(ctx, YH_E_INVALID, "%s: unknown mode %d", who, mode);
  if (!out) return fail(ctx, YH_E_INVALID, "%s: out is NULL", who);
  memcpy(planes, out, sizeof(yh_gbuffer));
  bool any = false;
  for (int k = 0; k < PLANES; k++) any = any || planes[k];
  if (!any) return fail(ctx, YH_E_INVALID, "%s: every plane is NULL", who);
  if (!lane_kernels_can_address(ctx))
    return fail(ctx, YH_E_INVALID, "%s: the one-lane form reads the scene's trees through 32-bit byte offsets and this scene's exceed 4 GB", who);
  return YH_OK;
}
}  // namespace

// for host/denoise.cpp, which traces its own guides: the pass into device planes (the caller has checked scene, state and pending launches)
int gbuffer_pass(yh_context* ctx, const char* who, int mode, void* const planes[PLANES]) {
  if (!lane_kernels_can_address(ctx))
    return fail(ctx, YH_E_INVALID, "%s: the one-lane form reads the scene's trees through 32-bit byte offsets and this scene's exceed 4 GB", who);
  return gbuffer_impl(ctx, who, mode, planes);
}

int yh_trace_gbuffer_device(yh_context* ctx, int mode, const yh_gbuffer* out) {
  if (!ctx) return YH_E_INVALID;
  void* planes[PLANES];
  if (int rc = gbuffer_checks(ctx, "yh_trace_gbuffer_device", mode, out, planes)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  return gbuffer_impl(ctx, "yh_trace_gbuffer_device", mode, planes);
}

int yh_trace_gbuffer(yh_context* ctx, int mode, const yh_gbuffer* out) {
  if (!ctx) return YH_E_INVALID;
  void* host[PLANES];
  if (int rc = gbuffer_checks(ctx, "yh_trace_gbuffer", mode, out, host)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  const size_t npix = (size_t)ctx->state.width * ctx->state.height;
  DevBuf       staged[PLANES];
  void*        planes[PLANES];
  for (int k = 0; k < PLANES; k++) {
    planes[k] = nullptr;
    if (!host[k]) continue;
    if (int rc = alloc_zero(ctx, staged[k], plane_bytes[k] * npix)) return rc;
    planes[k] = staged[k].p;
  }
  if (int rc = gbuffer_impl(ctx, "yh_trace_gbuffer", mode, planes)) return rc;
  for (int k = 0; k < PLANES; k++)
    if (host[k]) HIPCHK(ctx, hipMemcpy(host[k], planes[k], plane_bytes[k] * npix, hipMemcpyDeviceToHost));
  return YH_OK;
}
