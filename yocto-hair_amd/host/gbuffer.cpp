// gbuffer.cpp — yh_trace_gbuffer / yh_trace_gbuffer_device: the first-hit feature pass (unit/gbuffer.hip) over the image of yh_init_state.
#include "image_pass.h"

namespace {
// The pass into `out` (device pointers, NULL = skipped). Reads the render state, writes none of it.
int gbuffer_impl(yh_context* ctx, const char* who, int mode, const yh_gbuffer& out) {
  const int64_t npix  = (int64_t)ctx->state.width * ctx->state.height;
  const int64_t items = (int64_t)ctx->state.tiles_x * tiles_of(ctx->state.height) * 64;  // the cursor's range: whole 8x8 tiles
  if (items > (1ll << 30)) return fail(ctx, YH_E_INVALID, "%s: the image has too many pixels for the pass's 32-bit cursor", who);
  const int occupancy = std::min(yhk_gbuffer_waves(), yhk_gbuffer_occupancy(&ctx->scene));  // (256-thread blocks: one wave per SIMD each)
  if (occupancy < 1) return fail(ctx, YH_E_DEVICE, "%s: k_gbuffer cannot run with its LDS layout on this device", who);
  const int grid        = (int)std::max<int64_t>(1, std::min<int64_t>((npix + 255) / 256, (int64_t)ctx->num_cus * occupancy));
  const int ovf_entries = lane_overflow_entries(ctx);
  DevBuf    cursor, ovf;
  int       rc;
  if ((rc = alloc_zero(ctx, cursor, 16)) || (rc = alloc_zero(ctx, ovf, (size_t)grid * 4 * ovf_entries * 64 * 4))) return rc;
  const yhd_scene* sc_dev = nullptr;
  if ((rc = scene_copy(ctx, &sc_dev))) return rc;
  void* planes[PLANES];
  memcpy(planes, &out, sizeof(out));
  if ((rc = timed_begin(ctx))) return rc;
  int e = yhk_gbuffer(&ctx->scene, sc_dev, &ctx->state, mode, planes, (int*)cursor.p, (unsigned int*)ovf.p, ovf_entries, grid, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: k_gbuffer launch: %s", who, hipGetErrorString((hipError_t)e));
  return timed_end(ctx, 1);  // (yh_last_trace_ms: the kernel alone, without the copies)
}

int gbuffer_checks(yh_context* ctx, const char* who, int mode, const yh_gbuffer* out) {
  if (int rc = state_checks(ctx, who, NEED_SCENE | NEED_STATE)) return rc;
  if (mode != YH_GBUFFER_CENTRE && mode != YH_GBUFFER_NEXT_SAMPLE) return fail(ctx, YH_E_INVALID, "%s: unknown mode %d", who, mode);
  if (!out) return fail(ctx, YH_E_INVALID, "%s: out is NULL", who);
  if (!planes_present(*out)) return fail(ctx, YH_E_INVALID, "%s: every plane is NULL", who);
  if (!lane_kernels_can_address(ctx)) return refuse_lane_offsets(ctx, who);
  return YH_OK;
}
}  // namespace

// for the passes that trace their own guides (image_pass.cpp: trace_guides): the pass into device planes (the caller has checked scene, state and pending launches)
int gbuffer_pass(yh_context* ctx, const char* who, int mode, const yh_gbuffer& planes) {
  if (!lane_kernels_can_address(ctx)) return refuse_lane_offsets(ctx, who);
  return gbuffer_impl(ctx, who, mode, planes);
}

int yh_trace_gbuffer_device(yh_context* ctx, int mode, const yh_gbuffer* out) {
  if (!ctx) return YH_E_INVALID;
  if (int rc = gbuffer_checks(ctx, "yh_trace_gbuffer_device", mode, out)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  return gbuffer_impl(ctx, "yh_trace_gbuffer_device", mode, *out);
}

int yh_trace_gbuffer(yh_context* ctx, int mode, const yh_gbuffer* out) {
  if (!ctx) return YH_E_INVALID;
  if (int rc = gbuffer_checks(ctx, "yh_trace_gbuffer", mode, out)) return rc;
  if (int rc = enter_device(ctx)) return rc;
  const size_t npix = (size_t)ctx->state.width * ctx->state.height;
  Staged       s(ctx);
  yh_gbuffer   dev{};
  for (int k = 0; k < PLANES; k++)
    if (plane_of(*out, k)) set_plane(dev, k, s.out(plane_bytes[k] * npix));
  if (s.rc) return s.rc;
  if (int rc = gbuffer_impl(ctx, "yh_trace_gbuffer", mode, dev)) return rc;
  for (int k = 0; k < PLANES; k++)
    if (plane_of(*out, k)) HIPCHK(ctx, hipMemcpy(plane_of(*out, k), plane_of(dev, k), plane_bytes[k] * npix, hipMemcpyDeviceToHost));
  return YH_OK;
}
