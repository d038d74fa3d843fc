// trace_launch.cpp — yh_init_state (pt.cpp:1931-1946) and the launches of the sample-loop kernels: yh_trace_samples and friends.
#include "context_internal.h"

// Waits for everything queued on the context's stream, at most YHAIR_LAUNCH_TIMEOUT_S seconds (host/deadline.h): the blocking
// hipStreamSynchronize runs on the context's worker thread and this thread waits for it with the deadline, so that a kernel that never
// completes costs the caller an error, not the process. On expiry the context is POISONED: the device may still be running the kernel
// (and the worker is still inside the call), so every later call is refused and yh_destroy frees nothing (hipFree would wait too).
int wait_for_launch(yh_context* ctx) {
  if (ctx->poisoned) return refuse_poisoned(ctx);
  const double timeout = yhh::launch_timeout_s();
  const int    device  = ctx->device;
  hipStream_t  stream  = ctx->stream;
  int          e       = 0;
  // The blocking wait of the HIP runtime sleeps on an interrupt and wakes up tens of microseconds after the kernel has ended — for the bench's
  // 15 ms launches that was most of what the library added to a step (profiles/r05/bounded_wait_overhead.txt) — so the wait first SPINS for as
  // long as launches of this context have been taking (at most 50 ms, never past the deadline)
  // ... and for that long THIS thread asks the stream itself (hipStreamQuery: nothing blocks, nothing can hang): a launch of the usual length is
  // over before the question stops being asked, and the two thread hand-overs to the worker and back never happen.
  const double spin_s  = std::min(std::min(0.050, timeout), 1.25e-3 * (double)ctx->last_ms + 0.001);
  {
    const auto t0 = std::chrono::steady_clock::now();
    while (true) {
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) return YH_OK;
      if (q != hipErrorNotReady) return fail(ctx, YH_E_DEVICE, "hipStreamQuery: %s", hipGetErrorString(q));
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > spin_s) break;
    }
  }
  const int    rc      = ctx->sync_call.run(
      [device, stream]() {
        hipError_t se = hipSetDevice(device);
        return (int)(se != hipSuccess ? se : hipStreamSynchronize(stream));
      },
      timeout, &e);
  if (rc == yhh::WAIT_EXPIRED) {
    ctx->poisoned = true;
    return fail(ctx, YH_E_DEVICE, "the launch did not complete within %.3g s (YHAIR_LAUNCH_TIMEOUT_S): the context refuses further launches; destroy it and, to retry, start a fresh process", timeout);
  }
  if (e != (int)hipSuccess) return fail(ctx, YH_E_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString((hipError_t)e));
  return YH_OK;
}

int yh_init_state(yh_context* ctx, const yh_trace_params* params) {
  if (!ctx) return YH_E_INVALID;
  if (ctx->poisoned) return refuse_poisoned(ctx);
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "yh_init_state before yh_upload_scene");
  if (!params || params->resolution <= 0 || params->bounces < 0)
    return fail(ctx, YH_E_INVALID, "bad trace params");
  if (params->shader < 0 || params->shader >= YH_SHADER_COUNT)
    return fail(ctx, YH_E_INVALID, "sampler unknown");  // get_trace_shader_func's throw (pt.cpp:1669)
  if (params->hair_exact && params->shader != YH_SHADER_PATH) return fail(ctx, YH_E_INVALID, "hair_exact exists for the path shader only");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);  // (an asynchronous launch may still be running on the buffers this call replaces: wait for it, within the deadline)
  Lap        lap("init_state");
  const bool same_work = ctx->have_state && ctx->params.shader == params->shader && ctx->params.bounces == params->bounces;  // (what the items' relative costs depend on besides the image)
  ctx->params = *params;
  // image size (pt.cpp:1933-1939)
  auto& cam = ctx->scene.camera;
  int   w, h;
  if (cam.film_x > cam.film_y) {
    w = params->resolution;
    h = (int)round(params->resolution * cam.film_y / cam.film_x);
  } else {
    w = (int)round(params->resolution * cam.film_x / cam.film_y);
    h = params->resolution;
  }
  if (w <= 0 || h <= 0) return fail(ctx, YH_E_INVALID, "empty image");
  if (ctx->tp.have && (ctx->tp.width != w || ctx->tp.height != h)) temporal_drop(ctx);  // (the temporal history is another image's)
  size_t npix = (size_t)w * h;
  // per-pixel streams (pt.cpp:1942-1945), pixel order j * W + i
  std::vector<uint64_t> st(npix), inc(npix);
  Rng master = make_rng(1301081);
  for (size_t i = 0; i < npix; i++) {
    int seq = (int)(advance_rng(master) % 2147483648u) / 2 + 1;  // rand1i(rng, 1 << 31) / 2 + 1
    Rng r   = make_rng(params->seed, (uint64_t)seq);
    st[i] = r.state, inc[i] = r.inc;
  }
  lap("pixel streams (host)");
  int tx = tiles_of(w), ty = tiles_of(h);
  ctx->num_tiles_total = tx * ty;
  auto& owned = ctx->owned;
  owned.clear();
  for (int t = ctx->rank; t < ctx->num_tiles_total; t += ctx->world) owned.push_back(t);
  bool new_image = false;
  if ((int)ctx->item_cost.size() != ctx->num_tiles_total * 4) {  // scheduling hints survive a re-init of the same image
    ctx->item_cost.assign((size_t)ctx->num_tiles_total * 4, 0);
    ctx->item_scale.clear(), ctx->st_log_fresh = false;
    ctx->have_costs = false, ctx->costs_settled = false, ctx->dense = -1, ctx->chain = -1, ctx->chain16 = -1, ctx->launch_shape = YH_SHAPE_QUAD;
    for (double& t : ctx->shape_ms) t = 0;
    for (int& t : ctx->shape_trials) t = 0;
    new_image = true;
  }
  std::vector<int> tiles;
  build_work_items(ctx, tiles);
  const int first_shape = yhh::forced_shape() >= 0 ? yhh::forced_shape() : ctx->launch_shape;
  prepare_work_list(ctx, tiles, params->shader == YH_SHADER_PATH ? first_shape : YH_SHAPE_QUAD);
  tiles.reserve(4 * (size_t)ctx->num_tiles_total * 4 + 4);  // (the list's buffer holds the octet / sixteen-lane kernels' longer lists too)
  int rc;
  if ((rc = upload(ctx, ctx->d_rng_state, st.data(), npix * 8))) return rc;
  if ((rc = upload(ctx, ctx->d_rng_inc, inc.data(), npix * 8))) return rc;
  if ((rc = alloc_zero(ctx, ctx->d_accum, npix * 16))) return rc;
  if ((rc = alloc_zero(ctx, ctx->d_image, npix * 16))) return rc;
  {
    const size_t n = tiles.size();
    tiles.resize(std::max(n, 4 * owned.size() * 4), 0);
    if ((rc = upload(ctx, ctx->d_tiles, tiles.data(), tiles.size() * 4))) return rc;
    tiles.resize(n);
  }
  if ((rc = alloc_zero(ctx, ctx->d_counters, sizeof(yhd_counters)))) return rc;
  if ((rc = alloc_zero(ctx, ctx->d_tile_cursor, YH_TILE_CURSOR_BYTES))) return rc;
  if ((rc = alloc_zero(ctx, ctx->d_tile_cost, tile_cost_bytes(ctx)))) return rc;
  auto& s = ctx->state;
  s.tile_cursor = (int*)ctx->d_tile_cursor.p, s.tile_cost = (unsigned int*)ctx->d_tile_cost.p;
  s.rng_state = (uint64_t*)ctx->d_rng_state.p, s.rng_inc = (uint64_t*)ctx->d_rng_inc.p;
  s.accum = (yhd_float4*)ctx->d_accum.p, s.tiles = (const int*)ctx->d_tiles.p;
  s.launch_shape = first_shape;
  s.num_tiles = (int)tiles.size(), s.width = w, s.height = h, s.tiles_x = tx;
  if (new_image || !same_work) ctx->launches_of_image = 0;
  s.samples_done = 0, s.bounces = params->bounces, s.clamp = params->clamp, s.shader = params->shader;
  s.shard_rank = ctx->rank, s.shard_world = ctx->world;
  ctx->have_state = true;
  lap("work list, buffers, copies");
  if (new_image) trials_load(ctx);  // what this process already measured on this scene, image and shard
  // Probe: the first launch of a new image has no item costs and would hand its work items out in image order,
  // 25-60 % slower than a planned launch (hair quadrants cost 10-100x background ones and bound the launch when
  // they start last). One sample of every pixel measures them; the state is then put back as it was, so the
  // render starts planned and from the reference's RNG states. (YHAIR_NO_PROBE: developer switch.)
  bool measured = false;
  for (int t : owned)
    for (int q = 0; q < 4 && !measured; q++) measured = ctx->item_cost[(size_t)t * 4 + q] != 0;
  if (!measured && !owned.empty() && params->shader == YH_SHADER_PATH && !yhh::no_probe()) {
    ctx->state.launch_shape = YH_SHAPE_QUAD;
    int prc = trace_impl(ctx, 1, false, true);  // blocking; re-plans the hand-out order from the measured costs
    if (prc) return prc;
    HIPCHK(ctx, hipMemcpy(ctx->d_rng_state.p, st.data(), npix * 8, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_accum.p, 0, npix * 16, ctx->stream));
    YH_WAIT(ctx);
    ctx->state.samples_done = 0, ctx->launches_of_image = 0, ctx->last_shape = -1, ctx->last_ms = 0, ctx->last_launches = 0;
    ctx->have_costs = true;  // the launches that follow are planned: their times rank the kernels
    lap("probe launch + plan");
  }
  return YH_OK;
}

// The start of every sample-loop launch: the work list's cursors and the items' costs cleared, and the start event.
static int begin_launch(yh_context* ctx) {
  HIPCHK(ctx, hipMemsetAsync(ctx->d_tile_cursor.p, 0, YH_TILE_CURSOR_BYTES, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->d_tile_cost.p, 0, tile_cost_bytes(ctx), ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return YH_OK;
}
// The end of every sample-loop launch: its stop event and samples and, for a blocking one, the bounded wait, its time, what the
// kernel leaves to read back (`read_back`: k_stream's wave stamps) and the re-plan.
template <typename F>
static int end_launch(yh_context* ctx, int nsamples, bool sync, F&& read_back) {
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->state.samples_done += nsamples;
  ctx->last_launches = 1;
  if (!sync) return YH_OK;
  if (int wrc = wait_for_launch(ctx)) return wrc;
  HIPCHK(ctx, hipEventElapsedTime(&ctx->last_ms, ctx->ev0, ctx->ev1));
  if (int rc = read_back()) return rc;
  return replan_after_launch(ctx, nsamples);
}

// One launch of the streaming integrator (csrc/stream.hip): persistent wavefronts, one path pool each, one lane per path.
int stream_impl(yh_context* ctx, int nsamples, bool sync) {
  int  P = 0, grid = 0, lds_bytes = 0;
  bool one_generation = false;
  if (!lane_kernels_can_address(ctx))
    return fail(ctx, YH_E_INVALID, "k_stream (launch shape 3) reads the scene's trees through 32-bit byte offsets and this scene's exceed 4 GB: the quad kernels render it");
  if (!stream_geometry(ctx, ctx->st_items > 0 ? ctx->st_items : ctx->state.num_tiles, &P, &grid, &lds_bytes, &one_generation))
    return fail(ctx, YH_E_DEVICE, "k_stream cannot run with its LDS layout on this device");
  const int     wpb    = yhk_stream_block_threads() / 64;
  size_t        waves  = (size_t)grid * wpb;
  // The per-wave shares of the work list (deal_shares_by_speed) are made for ONE launch geometry — a wave count and a pool size — and the
  // cursor then starts behind the whole list: launched with another geometry (YHAIR_ST_WAVES / YHAIR_ST_SLOTS changed between the plan and
  // the launch), waves beyond the plan's would find nothing, shares beyond the pool's slots would be dropped, and samples_done would still
  // advance over pixels nobody rendered. So: a mismatch re-deals the list for the geometry of THIS launch; if that does not settle it, the
  // launch is refused — never a list the waves cannot reach.
  if (ctx->stream_pool.wave_begin && (ctx->st_share_waves != waves || ctx->st_share_slots != P)) {
    if (int wrc = wait_for_launch(ctx)) return wrc;
    if (int rc = upload_work_items(ctx)) return rc;
    if (!stream_geometry(ctx, ctx->st_items > 0 ? ctx->st_items : ctx->state.num_tiles, &P, &grid, &lds_bytes, &one_generation))
      return fail(ctx, YH_E_DEVICE, "k_stream cannot run with its LDS layout on this device");
    waves = (size_t)grid * wpb;
    if (ctx->stream_pool.wave_begin && (ctx->st_share_waves != waves || ctx->st_share_slots != P))
      return fail(ctx, YH_E_STATE, "k_stream: the work list was shared out for %zu waves of %d slots and the launch has %zu of %d", ctx->st_share_waves, ctx->st_share_slots, waves, P);
  }
  const size_t  slots  = waves * P;
  const int    ovf_entries = lane_overflow_entries(ctx);
  const size_t ovf_words   = waves * (size_t)ovf_entries * 64;
  int rc;
  if (slots > ctx->st_slots) {
    static_assert(sizeof(yhd_path_slot) == 128, "a path slot is one cache line");
    if ((rc = alloc_zero(ctx, ctx->d_st_slots, slots * sizeof(yhd_path_slot)))) return rc;
    ctx->st_slots          = slots;
    ctx->stream_pool.slots = (yhd_path_slot*)ctx->d_st_slots.p;
  }
  if (ctx->scene.general_materials && slots > ctx->st_medium_slots) {
    if ((rc = alloc_zero(ctx, ctx->d_st_medium, slots * 32))) return rc;
    ctx->st_medium_slots = slots, ctx->stream_pool.medium = (yhd_float4*)ctx->d_st_medium.p;
  }
  if (ovf_words > ctx->st_ovf_words) {
    if ((rc = alloc_zero(ctx, ctx->d_st_ovf, ovf_words * 4))) return rc;
    ctx->st_ovf_words = ovf_words, ctx->stream_pool.stack_ovf = (unsigned int*)ctx->d_st_ovf.p;
  }
  ctx->stream_pool.slots_per_wave = P, ctx->stream_pool.ovf_entries = ovf_entries, ctx->stream_pool.total_slots = (long long)ctx->st_slots;
  ctx->stream_pool.suspend_lanes  = one_generation ? 8 : 16;  // (csrc/stream.hip: YH_SUSPEND_LANES)
  const int prof = yhh::st_prof();  // developer switch: per-stage counters on stderr
  if (prof) {
    if ((rc = alloc_zero(ctx, ctx->d_st_prof, 64 * 8))) return rc;
    ctx->stream_pool.prof = (unsigned long long*)ctx->d_st_prof.p;
    ctx->stream_pool.prof_parts_only = prof == 2;
  } else {
    ctx->stream_pool.prof = nullptr;
  }
  // every launch keeps the waves' begin / end stamps and work (32 bytes per wave): the speeds of the hardware wave slots the next
  // hand-out is sized by (launch_plan.cpp: note_stream_wave_log); YHAIR_ST_WAVELOG prints their distribution
  const bool wave_log = yhh::st_wavelog();
  if (ctx->d_st_wave_log.bytes < waves * 16)
    if ((rc = alloc_zero(ctx, ctx->d_st_wave_log, waves * 16))) return rc;
  ctx->stream_pool.wave_log = (unsigned long long*)ctx->d_st_wave_log.p;
  ctx->stream_pool.wave_fill = nullptr;
  if (ctx->stream_pool.wave_begin) {
    if (ctx->d_st_wave_fill.bytes < waves * 4)
      if ((rc = alloc_zero(ctx, ctx->d_st_wave_fill, waves * 4))) return rc;
    ctx->stream_pool.wave_fill = (int*)ctx->d_st_wave_fill.p;
  }
  const yhd_scene* sc_dev = nullptr;
  if ((rc = scene_copy(ctx, &sc_dev))) return rc;
  if ((rc = begin_launch(ctx))) return rc;
  int e = yhk_stream(&ctx->scene, sc_dev, &ctx->state, nsamples, &ctx->stream_pool, grid, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "k_stream launch: %s", hipGetErrorString((hipError_t)e));
  return end_launch(ctx, nsamples, sync, [&]() -> int {
    std::vector<unsigned long long> w(waves * 2);
    HIPCHK(ctx, hipMemcpy(w.data(), ctx->d_st_wave_log.p, w.size() * 8, hipMemcpyDeviceToHost));
    note_stream_wave_log(ctx, w.data(), waves);
    if (wave_log) report_stream_waves(ctx, w.data(), waves, wpb);
    if (prof) return report_stream_prof(ctx, grid, wpb, P);
    return YH_OK;
  });
}

int trace_impl(yh_context* ctx, int nsamples, bool counted, bool sync) {
  if (!ctx) return YH_E_INVALID;
  if (ctx->poisoned) return fail(ctx, YH_E_DEVICE, "a launch of this context exceeded its deadline: the context refuses further launches, destroy it");
  if (!ctx->have_state) return fail(ctx, YH_E_STATE, "yh_trace_samples before yh_init_state");
  if (nsamples < 0) return fail(ctx, YH_E_INVALID, "negative sample count");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (nsamples == 0 || ctx->owned.empty()) {
    ctx->state.samples_done += nsamples;
    ctx->last_ms = 0, ctx->last_launches = 0;
    return YH_OK;
  }
  const bool path = ctx->state.shader == YH_SHADER_PATH;
  if (counted && !path) return fail(ctx, YH_E_INVALID, "work counters exist for the path shader only");
  if (settle_launch_shape(ctx, counted, nsamples, sync)) {  // the kernel for this launch; the hand-out order follows it
    // The list is rewritten by a blocking copy on the null stream; the context's stream is non-blocking, so a launch
    // queued by yh_trace_samples_async may still be reading it: wait for it first.
    if (int wrc = wait_for_launch(ctx)) return wrc;
    if (int rc = upload_work_items(ctx)) return rc;
  }
  const int shape = path ? ctx->state.launch_shape : YH_SHAPE_QUAD;  // the preview shaders have one launch shape
  ctx->last_shape = shape, ctx->last_counted = counted, ctx->planned_settled = ctx->costs_settled;
  const int kind = yhd_shapes[shape].kind;
  if (kind == YH_SHAPE_KIND_STREAM) return stream_impl(ctx, nsamples, sync);
  if (kind == YH_SHAPE_KIND_RETIRED) return fail(ctx, YH_E_INVALID, "launch shape 2 (quads over 8-wide nodes) was a developer kernel and is not built (profiles/r03/w8_oct_ab.txt)");
  if (kind == YH_SHAPE_KIND_SBS) return side_by_side_impl(ctx, nsamples, sync);  // (never counted: no instrumented build)
  int waves_per_block = yhk_block_threads(shape) / 64;  // one work item per wave at a time
  int lds_bytes       = yhk_trace_lds_bytes(&ctx->scene, shape);
  const bool exact    = path && ctx->params.hair_exact && !counted;
  int occupancy       = exact ? yhk_trace_exact_occupancy(lds_bytes, ctx->scene.general_materials) : yhk_trace_occupancy(lds_bytes, ctx->scene.general_materials, shape);
  if (occupancy < 1) return fail(ctx, YH_E_DEVICE, "k_trace cannot run with %d bytes of LDS per block", lds_bytes);
  int resident        = ctx->num_cus * occupancy;
  int want            = (ctx->state.num_tiles + waves_per_block - 1) / waves_per_block;
  int grid            = std::max(1, std::min(want, resident));
  if (int rc = begin_launch(ctx)) return rc;
  int e = exact ? yhk_trace_exact(&ctx->scene, &ctx->state, nsamples, lds_bytes, grid, ctx->stream)
                : yhk_trace(&ctx->scene, &ctx->state, nsamples, counted ? (yhd_counters*)ctx->d_counters.p : nullptr, shape, grid, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "k_trace launch: %s", hipGetErrorString((hipError_t)e));
  return end_launch(ctx, nsamples, sync, [] { return YH_OK; });
}
// One side-by-side launch: k_trace_sbs over the whole list — its first G_o workgroups the octet entries behind the quad items,
// the other G_q the quad items [0, hy_quad_items).
int side_by_side_impl(yh_context* ctx, int nsamples, bool sync) {
  int G_o = 0, G_q = 0;
  if (!side_by_side_grids(ctx, &G_o, &G_q)) return fail(ctx, YH_E_DEVICE, "k_trace_sbs cannot run with %d bytes of LDS per block", yhk_trace_sbs_lds_bytes(&ctx->scene));
  if (int rc = begin_launch(ctx)) return rc;
  int e = yhk_trace_sbs(&ctx->scene, &ctx->state, nsamples, G_o, ctx->hy_quad_items, ctx->hy_oct_entries, std::max(1, G_o + G_q), ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "k_trace_sbs launch: %s", hipGetErrorString((hipError_t)e));
  return end_launch(ctx, nsamples, sync, [] { return YH_OK; });
}
int yh_trace_samples(yh_context* ctx, int nsamples) {
  if (!ctx) return YH_E_INVALID;
  // a long request starts with the short trial launches of the kernels this image has not timed yet (pick_launch_shape)
  float ms = 0;
  int   launches = 0, remaining = nsamples;
  do {
    const int n  = (remaining >= 2 * YH_TRIAL_SPP && trial_pending(ctx)) ? YH_TRIAL_SPP : remaining;
    const int rc = trace_impl(ctx, n, false, true);
    if (rc) return rc;
    ms += ctx->last_ms, launches += ctx->last_launches, remaining -= n;
  } while (remaining > 0);
  ctx->last_ms = ms, ctx->last_launches = launches;
  return YH_OK;
}
int yh_trace_samples_async(yh_context* ctx, int nsamples) {
  const int rc = trace_impl(ctx, nsamples, false, false);
  if (ctx && rc == YH_OK) ctx->async_pending = ctx->last_launches > 0;
  return rc;
}
int yh_synchronize(yh_context* ctx) {
  if (!ctx) return YH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int wrc = wait_for_launch(ctx)) return wrc;
  if (ctx->async_pending) (void)hipEventElapsedTime(&ctx->last_ms, ctx->ev0, ctx->ev1);  // (a blocking call has its own sum)
  ctx->async_pending = false;
  return YH_OK;
}
int yh_launch_shape(const yh_context* ctx) { return ctx ? ctx->last_shape : YH_E_INVALID; }
int yh_kernel_trials(const yh_context* ctx, double* ms_per_sample, int* trials, int count) {
  if (!ctx || !ms_per_sample || !trials || count < 1) return YH_E_INVALID;
  for (int k = 0; k < count; k++) {
    ms_per_sample[k] = k < YH_SHAPES ? ctx->shape_ms[k] : 0.0;
    trials[k]        = k < YH_SHAPES ? ctx->shape_trials[k] : 0;
    if (std::isinf(ms_per_sample[k])) ms_per_sample[k] = -1.0;  // a candidate that cannot run on this device
  }
  return YH_SHAPES;
}
int yh_trials_pending(const yh_context* ctx) { return ctx ? (trial_pending(ctx) ? 1 : 0) : YH_E_INVALID; }
int yh_last_trace_ms(const yh_context* ctx, float* ms, int* launches) {
  if (!ctx) return YH_E_INVALID;
  if (ms) *ms = ctx->last_ms;
  if (launches) *launches = ctx->last_launches;
  return YH_OK;
}
int yh_trace_samples_counted(yh_context* ctx, int nsamples, yh_workcounts* out) {
  if (!ctx || !out) return YH_E_INVALID;
  if (!ctx->have_state) return fail(ctx, YH_E_STATE, "yh_trace_samples_counted before yh_init_state");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(ctx->d_counters.p, 0, sizeof(yhd_counters), ctx->stream));
  if (ctx->count_bound > 0) {
    // The items that count: the head of the cost-ordered list as build_work_items makes it from the costs at hand — by item, not by
    // place in the launch's list, whose head prepare_work_list lays out by wave slot.
    std::vector<int> items;
    build_work_items(ctx, items);
    std::vector<unsigned char> counted(ctx->item_cost.size(), 0);
    for (size_t k = 0; k < items.size() && k < (size_t)ctx->count_bound; k++) counted[(size_t)items[k]] = 1;
    if (int urc = upload_keep(ctx, ctx->d_counted_items, counted.data(), counted.size())) return urc;
    const unsigned char* flags = (const unsigned char*)ctx->d_counted_items.p;
    HIPCHK(ctx, hipMemcpyAsync((char*)ctx->d_counters.p + offsetof(yhd_counters, counted_items), &flags, sizeof(flags), hipMemcpyHostToDevice, ctx->stream));
    YH_WAIT(ctx);  // (`flags` is a local)
  }
  int rc = trace_impl(ctx, nsamples, true, true);
  if (rc) return rc;
  yhd_counters c;
  HIPCHK(ctx, hipMemcpy(&c, ctx->d_counters.p, sizeof(c), hipMemcpyDeviceToHost));
  out->samples = c.samples, out->rays = c.rays, out->nodes = c.nodes, out->seg_tests = c.seg, out->tri_tests = c.tri;
  out->hair_shades = c.hair, out->surf_shades = c.surf, out->env_lookups = c.envl, out->env_samples = c.envs;
  out->cyc_trace = c.cyc_trace, out->cyc_shade = c.cyc_shade, out->ticks_tile = c.cyc_tile, out->wave_iters = c.wave_iters;
  out->wave_steps = c.wave_steps, out->lane_steps = c.lane_steps, out->lane_iters = c.lane_iters;
  out->cyc_geom = c.c_geom, out->cyc_sample = c.c_sample, out->cyc_eval = c.c_eval, out->cyc_rest = c.c_rest;
  for (int k = 0; k < 10; k++) out->branch[k] = c.branch[k];
  for (int k = 0; k < 3 * YH_REGIONS; k++) ctx->last_regions[k] = c.region[k];
  return YH_OK;
}
int yh_set_count_bound(yh_context* ctx, int items) {
  if (!ctx || items < 0) return YH_E_INVALID;
  ctx->count_bound = items;
  return YH_OK;
}
int yh_shade_regions(const yh_context* ctx, uint64_t* out, int capacity) {
  if (!ctx || !out || capacity < 0) return YH_E_INVALID;
  for (int k = 0; k < capacity && k < 3 * YH_REGIONS; k++) out[k] = ctx->last_regions[k];
  return 3 * YH_REGIONS;
}
