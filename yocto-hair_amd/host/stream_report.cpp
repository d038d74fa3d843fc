// stream_report.cpp — what the developer switches print about a launch, out of the launch path: YHAIR_ST_WAVELOG's and YHAIR_ST_PROF's
// reports of a k_stream launch (stream_impl calls them after a blocking launch) and the laps of YHAIR_TIMING. The printed text is read by
// tools/branch_budget.py, tools/shard_ab.py, tools/stream_step_parts.sh and tools/gpu_check.sh.
#include "context_internal.h"

// the ends of the previous launch's waves as fractions of its span, for the correlation line
static std::vector<double> g_prev_ends;

// The distribution of the waves' begin / end stamps (two per wave) over the launch's span.
void report_stream_waves(const yh_context* ctx, const unsigned long long* w, size_t waves, int wpb) {
  unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < waves; i++) t0 = std::min(t0, w[2 * i]), t1 = std::max(t1, w[2 * i + 1]);
  const double span = (double)(t1 - t0);
  // by hardware wave slot (= dispatch round of the wave's workgroup: num_cus workgroups per round) and by XCC (workgroup % 8)
  double sum_slot[16] = {}, n_slot[16] = {}, sum_x[8] = {}, n_x[8] = {}, start_slot[16] = {};
  std::vector<double> ends;
  double resident = 0;
  for (size_t i = 0; i < waves; i++) {
    const size_t blk = i / wpb;
    const int    sl = (int)std::min<size_t>(15, blk / ctx->num_cus), x = (int)(blk % 8);
    const double e = (double)(w[2 * i + 1] - t0) / span, b = (double)(w[2 * i] - t0) / span;
    sum_slot[sl] += e, n_slot[sl] += 1, sum_x[x] += e, n_x[x] += 1, start_slot[sl] += b;
    ends.push_back(e), resident += e - b;
  }
  {  // do the same waves end late launch after launch? correlation of the end stamps with the previous launch's (same wave count)
    const std::vector<double>& prev = g_prev_ends;
    if (prev.size() == ends.size()) {
      double ma = 0, mb = 0, saa = 0, sbb = 0, sab = 0;
      for (size_t i = 0; i < ends.size(); i++) ma += ends[i], mb += prev[i];
      ma /= ends.size(), mb /= ends.size();
      for (size_t i = 0; i < ends.size(); i++) saa += (ends[i] - ma) * (ends[i] - ma), sbb += (prev[i] - mb) * (prev[i] - mb), sab += (ends[i] - ma) * (prev[i] - mb);
      fprintf(stderr, "[yhair]   correlation of the waves' ends with the previous launch's: %.3f\n", sab / std::sqrt(std::max(1e-30, saa * sbb)));
    }
    g_prev_ends = ends;
  }
  std::sort(ends.begin(), ends.end());
  fprintf(stderr, "[yhair] k_stream wave log: %zu waves, span %.2f ms; a wave is resident %.3f of the span on average; ends at p10 %.3f p50 %.3f p90 %.3f p99 %.3f\n", waves,
      span / 1e5, resident / waves, ends[waves / 10], ends[waves / 2], ends[waves * 9 / 10], ends[waves * 99 / 100]);
  for (int k = 0; k < 16; k++)
    if (n_slot[k] > 0) fprintf(stderr, "[yhair]   dispatch round %d: %4.0f waves, begin %.3f, mean end %.3f\n", k, n_slot[k], start_slot[k] / n_slot[k], sum_slot[k] / n_slot[k]);
  fprintf(stderr, "[yhair]   mean end by XCC:");
  for (int k = 0; k < 8; k++) fprintf(stderr, " %.3f", n_x[k] > 0 ? sum_x[k] / n_x[k] : 0.0);
  fprintf(stderr, "\n");
}

// The counters of the instrumented k_stream (csrc/stream.hip), read back from d_st_prof: per stage, per part of a step, per branch.
int report_stream_prof(yh_context* ctx, int grid, int wpb, int P) {
  unsigned long long c[64];
  HIPCHK(ctx, hipMemcpy(c, ctx->d_st_prof.p, sizeof(c), hipMemcpyDeviceToHost));
  const char* names[6] = {"items", "sort", "finish", "hair", "surf", "trace"};
  double total = 0;
  for (int k = 0; k < 6; k++) total += (double)c[k];
  fprintf(stderr, "[yhair] k_stream %.2f ms, grid %d x %d waves, %d slots per wave\n", ctx->last_ms, grid, wpb, P);
  for (int k = 0; k < 6; k++)
    fprintf(stderr, "[yhair]   %-7s %5.1f %% of wave time, %9llu trips, mean batch %.1f lanes\n", names[k], 100.0 * (double)c[k] / total,
        c[8 + k], c[8 + k] ? (double)c[16 + k] / (double)c[8 + k] : 0.0);
  fprintf(stderr, "[yhair]   trace: %llu wave steps, %.1f lanes busy on average, %.0f cycles per step\n", c[24],
      c[24] ? (double)c[25] / (double)c[24] : 0.0, c[24] ? (double)c[5] / (double)c[24] : 0.0);
  {  // the five parts of a step (csrc/dev_lane.h: stamp), shader-clock cycles per wave step
    const char* part[5] = {"head (pop, scene level, ENTER)", "own loads, exchange, segment loads issued", "ray pulls, the wait for memory, node code", "the wave's line tests",
        "results back, accept"};
    double      sum = 0;
    for (int k = 0; k < 5; k++) sum += (double)c[52 + k];
    for (int k = 0; k < 5 && c[24]; k++)
      fprintf(stderr, "[yhair]   step part %d %-46s %7.0f cycles per step (%4.1f %% of the stamped step)\n", k, part[k], (double)c[52 + k] / (double)c[24], sum > 0 ? 100.0 * (double)c[52 + k] / sum : 0.0);
  }
  // per branch of lane_step (csrc/dev_lane.h: LP_*): the share of the wave steps that ran it, and the lanes in it when it ran
  const char* br[10] = {"step", "pop", "scene", "enter", "fetch", "node", "line-leaf", "tri-leaf", "push", "2nd-seg"};
  for (int b = 0; b < 10; b++)
    fprintf(stderr, "[yhair]   branch %-9s ran in %5.1f %% of the wave steps (%llu times), %.1f lanes on average\n", br[b],
        c[32] ? 100.0 * (double)c[32 + 2 * b] / (double)c[32] : 0.0, c[32 + 2 * b], c[32 + 2 * b] ? (double)c[33 + 2 * b] / (double)c[32 + 2 * b] : 0.0);
  return YH_OK;
}

void Lap::operator()(const char* what) {
  if (!on) return;
  auto now = std::chrono::steady_clock::now();
  fprintf(stderr, "[yhair] %s: %-28s %8.1f ms\n", prefix, what, std::chrono::duration<double, std::milli>(now - t_last).count());
  t_last = now;
}
