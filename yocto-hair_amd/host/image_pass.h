// image_pass.h — what the passes over the state's image share (gbuffer.cpp, denoise.cpp, temporal.cpp; bodies: image_pass.cpp): the
// refusals about the context's state, staging of host arrays, guide planes traced or staged on the device (by name: image_planes.h), the
// timed bracket behind yh_last_trace_ms, and the tone-mapped tail of the display entries.
#ifndef YH_IMAGE_PASS_H_
#define YH_IMAGE_PASS_H_
#include "context_internal.h"
#include "image_planes.h"
#include "../unit/variance_launchers.h"  // (the variance stage's kernels, declared outside csrc/: the reason is in that header)

#pragma GCC visibility push(hidden)  // internal to libyhair.so
// ---- refusals, before anything is written ----
constexpr int64_t MAX_PIXELS = 1ll << 28;
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// The run every entry has its part of, in this order: poisoned, no scene, no state, asynchronous launch pending, the own render on a shard.
enum : unsigned { CHECK_POISONED = 1, NEED_SCENE = 2, NEED_STATE = 4, OWN_RENDER = 8 };
int state_checks(yh_context* ctx, const char* who, unsigned checks);
inline int refuse_unaligned(yh_context* ctx, const char* who) { return fail(ctx, YH_E_INVALID, "%s: the float4 images must be 16-byte aligned", who); }
inline int refuse_too_many_pixels(yh_context* ctx, const char* who) { return fail(ctx, YH_E_INVALID, "%s: the image has too many pixels", who); }  // more than MAX_PIXELS
// lane_kernels_can_address(ctx) is false; `unit`: "form" or "kernel", as the entry has always said
inline int refuse_lane_offsets(yh_context* ctx, const char* who, const char* unit = "form") {
  return fail(ctx, YH_E_INVALID, "%s: the one-lane %s reads the scene's trees through 32-bit byte offsets and this scene's exceed 4 GB", who, unit);
}
int enter_device(yh_context* ctx);  // what follows the refusals: the context's device made current, whatever it has queued waited for

// ---- staging: device buffers that live as long as the object, one rc for all of them ----
struct Staged {
  std::vector<DevBuf> bufs;
  yh_context*         ctx;
  int                 rc = YH_OK;
  explicit Staged(yh_context* c) : ctx(c) { bufs.reserve(16); }
  void* in(const void* src, size_t bytes) { return add(bytes, src, 0); }  // upload: a bounded wait, then the copy
  void* out(size_t bytes) { return add(bytes, nullptr, 1); }              // alloc_zero: zeroed and waited for
  void* scratch(size_t bytes) { return add(bytes, nullptr, 2); }          // dev_alloc: no memset, no wait
  void* add(size_t bytes, const void* src, int kind);
};
// the planes of `mask` as device scratch in `s` (guide_order), to `dev`; stage_guides: with `host`'s content, copied after the last allocation
int scratch_guides(Staged& s, unsigned mask, size_t npix, yh_gbuffer& dev);
int stage_guides(Staged& s, unsigned mask, const yh_gbuffer& host, size_t npix, yh_gbuffer& dev);
// ... traced: the centre-mode feature pass over the state's image into them (sets yh_last_trace_ms as gbuffer_pass does)
int trace_guides(Staged& s, const char* who, unsigned mask, yh_gbuffer& dev);

// ---- timing: the event pair around a call's kernels, and the sum over the stages of a composite entry ----
int timed_begin(yh_context* ctx);                // records ev0
int timed_stop(yh_context* ctx);                 // records ev1 (what follows on the stream is not timed)
int timed_read(yh_context* ctx, int launches);   // waits; yh_last_trace_ms = ev0 .. ev1, with its launch count
int timed_end(yh_context* ctx, int launches);    // the two in one
struct PassTime {
  float ms = 0;
  int   launches = 0;
  void add(yh_context* ctx) { ctx->last_ms = ms += ctx->last_ms, ctx->last_launches = launches += ctx->last_launches; }  // the stage just run; the context reports the sum so far
};

// ---- the display entries ----
// d_display holds the state's image as bytes (wait_first: the device may still read the old one)
int ensure_display(yh_context* ctx, bool wait_first);
// the tone map of the float4 device image `d_img` into d_display (ensured by the caller), timed as a stage of `t`, copied to rgba8, waited for
int display_tail(yh_context* ctx, const char* who, const void* d_img, float exposure, int filmic, int srgb, uint8_t* rgba8, PassTime& t);

// ---- the temporal history (temporal.cpp), for the variance stage (variance.cpp) that advances it too ----
// TEMPORAL's refusals with the guide planes of `planes`; one step over given device planes, and one with the guides traced where `guides`
// is NULL. vp NULL: the plain step; else stages M and S of include/yhair.h: VARIANCE, the variance kept in ctx->tp.d_var and copied to
// d_var_out where that is not NULL.
int temporal_checks(yh_context* ctx, const char* who, const yh_temporal_params* p, bool own_render, int samples_in, const yh_gbuffer* guides, unsigned planes);
int temporal_step(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer& g, void* d_out,
    const yh_variance_params* vp, float* d_var_out);
int temporal_accumulate(yh_context* ctx, const char* who, const yh_temporal_params& P, const void* d_in, int samples, const yh_gbuffer* guides, void* d_out,
    const yh_variance_params* vp, float* d_var_out);
#pragma GCC visibility pop
#endif
