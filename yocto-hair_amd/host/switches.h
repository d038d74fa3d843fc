// switches.h — every YHAIR_* environment variable libyhair.so and its command lines read, one small accessor each. This is the one place
// that calls getenv("YHAIR_...").
//
// THE RULE: every accessor reads the environment WHEN IT IS CALLED. Nothing is cached in a static and nothing is copied into the context
// at yh_create: the tests set switches between calls on a live context, and a getenv per launch costs nothing next to a launch.
//
// | variable                  | values                  | what it does                                                                       | read by                                   |
// |---------------------------|-------------------------|------------------------------------------------------------------------------------|-------------------------------------------|
// | YHAIR_SHAPE               | 0 .. YH_SHAPES-1        | every launch runs that launch shape (or its fallback); no timing trials            | launch_plan.cpp, trace_launch.cpp         |
// | YHAIR_NO_TRIALS           | set                     | kernel choice by the cost heuristic only                                           | launch_plan.cpp (trials_off)              |
// | YHAIR_NO_TRIAL_CACHE      | set                     | forget the trial record, the per-process one and the one on disk                   | launch_plan.cpp                           |
// | YHAIR_NO_DISK_CACHE       | set                     | never read or write the trial record on disk, whatever directory was named         | launch_plan.cpp (disk_cache_path)         |
// | YHAIR_CACHE_DIR           | a directory             | keep the trial record on disk there (wins over yh_set_trial_cache_dir)             | launch_plan.cpp (disk_cache_path)         |
// | YHAIR_DEVICE_SHARE        | k >= 1                  | k processes render on this device at once: plan for a k-th of the waves; its text  | launch_plan.cpp (dense_by_costs, disk_key)|
// |                           |                         | is part of the key of the trial record on disk                                     |                                           |
// | YHAIR_LAUNCH_TIMEOUT_S    | seconds > 0 (1800)      | the deadline of every wait for the device (deadline.h)                             | trace_launch.cpp (wait_for_launch)        |
// | YHAIR_NO_PROBE            | set                     | no 1-spp probe launch at yh_init_state                                             | trace_launch.cpp                          |
// | YHAIR_INTERSECT           | quad, lane4 .. lane8    | yh_intersect_batch: the quad kernel, or the one-lane kernel at that many waves     | batch_api.cpp                             |
// | YHAIR_BVH                 | host, device            | build every shape on the host, or every shape on the device                        | scene_upload.cpp (shape_builds_on_device) |
// | YHAIR_GATHER              | rccl, peer              | yh_gather_framebuffer: force the collective (also for one context) or peer copies  | gather.cpp                                |
// | YHAIR_ST_SLOTS            | 64 .. 4096, step 64     | k_stream: pool slots per wave (and no one-generation launch)                       | launch_plan.cpp (stream_geometry)         |
// | YHAIR_ST_WAVES            | waves per CU            | k_stream: at most that many resident waves per CU                                  | launch_plan.cpp (stream_geometry)         |
// | YHAIR_ST_PROF             | 0, 1, 2                 | k_stream's instrumented build: 1 counters per stage and branch on stderr, 2 the    | trace_launch.cpp (stream_impl),           |
// |                           |                         | five time stamps of a step only; its launches rank no kernel                       | launch_plan.cpp (record_launch)           |
// | YHAIR_ST_WAVELOG          | set                     | the distribution of k_stream's wave stamps on stderr after every launch            | trace_launch.cpp (stream_impl)            |
// | YHAIR_TIMING              | 0, non-zero             | stage times of upload and yh_init_state, kernel-choice decisions, requests on      | Lap (stream_report.cpp), launch_plan.cpp, |
// |                           |                         | stderr                                                                             | yscenetrace.cpp                           |
//
// Two things were not the same at every site before this header; they are settled here, and are its only intended changes of behaviour:
//   * YHAIR_TIMING means "set and non-zero" everywhere (some sites took "set": YHAIR_TIMING=0 printed half of the lines);
//   * YHAIR_ST_PROF, YHAIR_DEVICE_SHARE and YHAIR_NO_TRIALS are read per call like the rest (some sites froze them at first use).
// (YHAIR_LIB — the Python binding's — and YHAIR_SCENES — bench.py's and the tests' — are not the library's.)
//
// Header-only and free of HIP: tests/cpp/ compiles it with g++ alone.
#ifndef YH_SWITCHES_H_
#define YH_SWITCHES_H_
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../csrc/yh_device.h"  // YH_SHAPES

namespace yhh {

// YHAIR_SHAPE=s: every launch runs shape s, or its fallback (settle_launch_shape); -1 when unset
inline int forced_shape() { const char* e = getenv("YHAIR_SHAPE"); return e ? std::max(0, std::min(YH_SHAPES - 1, atoi(e))) : -1; }
// YHAIR_NO_TRIALS: the cost heuristic only
inline bool no_trials() { return getenv("YHAIR_NO_TRIALS") != nullptr; }
// YHAIR_NO_TRIAL_CACHE: neither the per-process trial record nor the one on disk
inline bool no_trial_cache() { return getenv("YHAIR_NO_TRIAL_CACHE") != nullptr; }
// YHAIR_NO_DISK_CACHE: switches the record on disk off whatever was set
inline bool no_disk_cache() { return getenv("YHAIR_NO_DISK_CACHE") != nullptr; }
// YHAIR_CACHE_DIR: the directory of the record on disk; NULL when unset
inline const char* cache_dir() { return getenv("YHAIR_CACHE_DIR"); }

// YHAIR_DEVICE_SHARE=k: k processes render on this device at once (bench.py with more ranks than devices): a k-th of the waves is ours
inline int device_share() { const char* e = getenv("YHAIR_DEVICE_SHARE"); return std::max(1, e ? atoi(e) : 1); }
// ... and as the key of the trial record on disk spells it: the variable's text, "1" when unset
inline const char* device_share_key() { const char* e = getenv("YHAIR_DEVICE_SHARE"); return e ? e : "1"; }

// YHAIR_LAUNCH_TIMEOUT_S (seconds, fractions allowed; <= 0 or unparsable: the default). Read at every wait: a test sets it per call.
inline double launch_timeout_s() {
  const char* e = getenv("YHAIR_LAUNCH_TIMEOUT_S");
  if (e && *e) {
    char*        end = nullptr;
    const double v   = strtod(e, &end);
    // (clamped: duration<double> -> the condition variable's integer nanoseconds overflows above ~9.2e9 s, and a deadline in the past would
    // poison a healthy context at its first long wait; 1e8 s = three years is "never")
    if (end != e && v > 0) return v < 1e8 ? v : 1e8;
  }
  return 1800.0;
}

// YHAIR_NO_PROBE: yh_init_state plans a new image without its 1-spp probe launch
inline bool no_probe() { return getenv("YHAIR_NO_PROBE") != nullptr; }

// YHAIR_INTERSECT=quad | lane4 | lane5 | lane6 | lane8: yh_intersect_batch's kernel (waves: per SIMD of the lane kernel, clamped to 4 .. 8).
// Anything else, or unset: the batch decides, five waves (91 registers without a spill; 6 and 8 spill 39 / 61 registers, measured slower).
struct IntersectSwitch {
  enum { AUTO, QUAD, LANES } mode;
  int         waves;
  const char* text;  // the variable as set (for messages), NULL when unset
};
inline IntersectSwitch intersect_switch() {
  const char* e = getenv("YHAIR_INTERSECT");
  if (e && !strcmp(e, "quad")) return {IntersectSwitch::QUAD, 5, e};
  if (e && !strncmp(e, "lane", 4)) return {IntersectSwitch::LANES, std::max(4, std::min(8, atoi(e + 4))), e};
  return {IntersectSwitch::AUTO, 5, e};
}

// YHAIR_BVH=host: every shape is built the small shapes' way, on the host; YHAIR_BVH=device: every shape on the device
enum BvhSwitch { BVH_BY_SIZE, BVH_HOST, BVH_DEVICE };
inline BvhSwitch bvh_switch() {
  const char* e = getenv("YHAIR_BVH");
  return e && !strcmp(e, "host") ? BVH_HOST : e && !strcmp(e, "device") ? BVH_DEVICE : BVH_BY_SIZE;
}

// YHAIR_GATHER=peer: device-to-device copies even between distinct devices; YHAIR_GATHER=rccl: the collective even for ONE context
// (a communicator of one rank: how a one-GPU box executes the RCCL calls, tests/test_gpu_parity.py)
enum GatherSwitch { GATHER_BY_DEVICES, GATHER_RCCL, GATHER_PEER };
inline GatherSwitch gather_switch() {
  const char* e = getenv("YHAIR_GATHER");
  return e && !strcmp(e, "rccl") ? GATHER_RCCL : e && !strcmp(e, "peer") ? GATHER_PEER : GATHER_BY_DEVICES;
}

// YHAIR_ST_SLOTS: k_stream's pool slots per wave, a multiple of 64 in [64, 4096]; 0 when unset (stream_geometry chooses)
inline int st_slots() { const char* e = getenv("YHAIR_ST_SLOTS"); return e ? std::max(64, std::min(4096, atoi(e) / 64 * 64)) : 0; }
// YHAIR_ST_WAVES: at most that many resident waves of k_stream per CU — `occupancy` (workgroups of `waves_per_block` waves per CU) cut
// down to it, one workgroup at least; `occupancy` itself when unset
inline int st_occupancy(int occupancy, int waves_per_block) {
  const char* e = getenv("YHAIR_ST_WAVES");
  return e ? std::max(1, std::min(occupancy, (atoi(e) + waves_per_block - 1) / waves_per_block)) : occupancy;
}
// YHAIR_ST_PROF: k_stream's instrumented build. 0: off (unset, 0, not a number); 2: the five time stamps of a step only
// (tools/stream_step_parts.sh); 1 (any other number): the counters per stage and per branch of the step too
inline int st_prof() { const char* e = getenv("YHAIR_ST_PROF"); const int v = e ? atoi(e) : 0; return v == 0 ? 0 : v == 2 ? 2 : 1; }
// YHAIR_ST_WAVELOG: the distribution of k_stream's wave stamps on stderr (every launch keeps the stamps; this prints them)
inline bool st_wavelog() { return getenv("YHAIR_ST_WAVELOG") != nullptr; }

// YHAIR_TIMING: set and non-zero — stage times and kernel-choice decisions on stderr
inline bool timing() { const char* e = getenv("YHAIR_TIMING"); return e && atoi(e) != 0; }

}  // namespace yhh
#endif
