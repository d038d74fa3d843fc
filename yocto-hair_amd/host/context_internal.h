// context_internal.h — what the translation units of the host library share: the launchers of the .hip files (csrc/launchers.h), the context, small
// host helpers with the reference's operation order, and the internal functions that cross files. Not installed; the public
// interface is include/yhair.h.
//   context.cpp        create / destroy, errors, shard, downloads (yh_download_display: unit/display.hip)
//   scene_upload.cpp   yh_upload_scene = init_bvh + init_lights (pt.cpp:755-818,1695-1740): reference-identical BVHs, leaf-ordered
//                      records, inverse frames, per-material hair constants, light CDFs; the wide-node and lane-blob arrays — a list of
//                      stages (UploadStage); the ones without a HIP call are upload_stages.h, the traversal array's layout blob_layout.h
//   launch_plan.cpp    which kernel runs (timing trials, their record in memory and on disk) and the hand-out order of the work items
//   trace_launch.cpp   yh_init_state (pt.cpp:1931-1946) and the launches: yh_trace_samples and friends
//   stream_report.cpp  what the developer switches print about a launch (YHAIR_ST_WAVELOG, YHAIR_ST_PROF) and the laps of YHAIR_TIMING
//   (switches.h: every YHAIR_* environment variable, one accessor each)
//   gather.cpp         tile packing and the one collective (yh_gather_framebuffer: RCCL or peer copies)
//   batch_api.cpp      the unit-level batch entry points (hair BSDF, intersection, BVH build, curves, self-tests)
//   gbuffer.cpp        yh_trace_gbuffer / _device: the first-hit feature pass over the state's image (unit/gbuffer.hip)
//   denoise.cpp        yh_denoise and friends: the a-trous filter over the resolved render, guided by that pass (unit/denoise.hip, unit/atrous_math.h)
//   temporal.cpp       yh_temporal_accumulate and friends: the previous step's render reprojected into the new view and blended by sample
//                      count, in front of that filter (unit/reproject.hip, unit/reproject_math.h); the history it keeps between steps
//   image_pass.cpp     what those three share (image_pass.h): the state refusals, staging (Staged, also batch_api.cpp's), guide planes traced
//                      or staged by name (image_planes.h: the planes of yh_gbuffer and which of them a stage reads), timing, the display tail
//   scene_edit.cpp     edits of an uploaded scene that keep its geometry: yh_update_camera / _materials / _environments / _objects, and the
//                      scene level again (the tree over the objects' world boxes, which the shape edits move too)
//   shape_edit.cpp     one shape's vertices: yh_update_shape / _device (its tree again), yh_refit_shape / _device (that tree's boxes only,
//                      unit/refit.hip); yh_shape_nodes, yh_shape_refit_growth
//   light_edit.cpp     yh_set_light_edits: the light list again where an edit changes it (unit/light_list.hip; the rule itself:
//                      light_layout.h, shared with the upload); yh_light_list, yh_triangle_cdf / _gpu
//   (edit_internal.h: what crosses those three and the upload; light_layout.h, blob_layout.h: the two layouts both sides follow)
#ifndef YH_CONTEXT_INTERNAL_H_
#define YH_CONTEXT_INTERNAL_H_
#include <hip/hip_runtime_api.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rccl/rccl.h>  // types only: the library is opened on first use (yh_gather_framebuffer)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <tuple>
#include <string>
#include <memory>
#include <thread>
#include <vector>

#include "../csrc/yh_device.h"
#include "../csrc/launchers.h"    // every yhk_* launcher of csrc/*.hip and unit/*.hip: the declarations their definitions compile too
#include "../unit/object_math.h" // F3 and its helpers, inverse_frame, transform_point, transform_bbox, padded_world_box: shared with the device
#include "../unit/light_math.h"   // triangle_area: an area light's cdf entry, shared with the device
#include "../unit/light_list.h"   // yhk_light_job
#include "bvh_build.h"
#include "deadline.h"
#include "parallel_for.h"
#include "switches.h"
#include "yhair.h"

// A device allocation owned by the context.
struct DevBuf {
  void*  p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;  // owns a hipMalloc pointer
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr, bytes = 0;
  }
  void swap(DevBuf& o) { std::swap(p, o.p), std::swap(bytes, o.bytes); }
};

namespace {



const float pif = (float)3.14159265358979323846;

// PCG32 (math.h:1396-1442) for init_state and the self-test drivers
struct Rng {
  uint64_t state, inc;
};
uint32_t advance_rng(Rng& rng) {
  uint64_t old        = rng.state;
  rng.state           = old * 6364136223846793005ULL + rng.inc;
  uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
  uint32_t rot        = (uint32_t)(old >> 59u);
  return (xorshifted >> rot) | (xorshifted << ((-rot) & 31));
}
Rng make_rng(uint64_t seed, uint64_t seq = 1) {
  Rng rng{0, (seq << 1u) | 1u};
  advance_rng(rng);
  rng.state += seed;
  advance_rng(rng);
  return rng;
}
float rand1f(Rng& rng) {
  uint32_t u = (advance_rng(rng) >> 9) | 0x3f800000u;
  float    f;
  memcpy(&f, &u, 4);
  return f - 1.0f;
}
void skip_rng(Rng& rng, uint64_t delta) {  // LCG jump-ahead
  uint64_t cur_mult = 6364136223846793005ULL, cur_plus = rng.inc, acc_mult = 1u, acc_plus = 0u;
  while (delta > 0) {
    if (delta & 1) acc_mult *= cur_mult, acc_plus = acc_plus * cur_mult + cur_plus;
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta /= 2;
  }
  rng.state = acc_mult * rng.state + acc_plus;
}

float sqr(float v) { return v * v; }
template <int N>
float powt(float v) {  // ext.cpp:95-109
  if constexpr (N == 0) return 1;
  else if constexpr (N == 1) return v;
  else {
    float n2 = powt<N / 2>(v);
    return n2 * n2 * powt<(N & 1)>(v);
  }
}

}  // namespace

struct yh_context {
  int         device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t  ev0 = nullptr, ev1 = nullptr;
  int         hy_quad_items = 0, hy_oct_entries = 0;  // layout of the work list for YH_SHAPE_SBS: [quad items][octet entries]
  std::vector<int> hy_oct_items;                       // ... and the items that run as octets
  int         num_cus = 0;
  std::string device_name;  // gcnArchName / marketing name / CU count: part of the key of the trial record on disk
  std::string error = "no error";
  yhh::BoundedCall sync_call;    // the blocking hipStreamSynchronize of this context's stream, on a worker thread with a deadline (wait_for_launch)
  bool        poisoned = false;  // a launch of this context did not complete within its deadline (wait_for_launch): no further launches, nothing is freed
  // scene
  bool      have_scene = false;
  yhd_scene scene{};
  DevBuf    d_prims, d_vpos, d_elems, d_objects, d_materials, d_scene_nodes,
      d_scene_prims, d_light_cdf, d_env_texels, d_light_table, d_env_tab;
  int       stack_need = 0, stack_need8 = 0, stack_need16 = 0;
  // where every shape's test records and nodes sit in the traversal kernels' array (yhd_scene::lane_blob), made at yh_upload_scene
  struct LaneShape { int kind, num_nodes, prim_base, num_prims; long long node_off, test_off, node_off8, node_off16; };  // offsets in 32-byte units: the shape's 4- / 8- / 16-wide nodes and its test records
  std::vector<LaneShape>   lane_shapes;
  long long                lane_units = 0;
  DevBuf                   d_lane_blob;
  // what an edit of the uploaded scene needs of its description (host/edit_internal.h): the material rows as they were passed in, their maps
  // (empty: no material has an effective map) with the device's records of them, whether some area light is read through memory (one of
  // the inputs of yhd_scene::general_materials), and the bytes the fingerprint mixes in its order — camera, materials, objects and
  // geometry sample, environment heads, maps
  std::vector<yh_material>      h_materials;
  std::vector<yh_material_maps> h_maps;
  std::vector<yhd_maps>         h_dmaps;
  bool                          big_lights = false;
  // yh_set_light_edits: the edits make the light list again instead of refusing what changes it; and the texel cdf of every textured
  // environment that has been a light since the upload, kept on the device (made with the host's sine: off and on again costs a copy)
  bool                          light_edits = false;
  DevBuf                        d_env_cdf[YH_MAX_ENVS];
  yh_camera                     key_camera{};
  std::vector<unsigned char>    key_geometry, key_envs;
  // ... and what yh_update_objects needs of the upload: every shape's root box (on the device too, 6 floats per shape: unit/objects.hip
  // reads it), the deepest shape tree as 4- / 8- / 16-wide nodes, every object's world box (the scene tree is built over all of them),
  // and how many 4-wide scene nodes the front of the lane blob has room for (0: the scene level is not walked from there)
  std::vector<yhh::Box>         h_shape_roots, h_obj_boxes;
  DevBuf                        d_shape_roots;
  int                           max_shape_depth = 0, max_shape_depth8 = 0, max_shape_depth16 = 0;
  int                           scene_wide_room = 0;
  // ... and what yh_update_shape needs of every shape: what its counts and arrays were, where its per-vertex rows sit (per_vertex: it has
  // some), the depths of its tree as 4- / 8- / 16-wide nodes (the maxima above are made from them again), how many nodes of each width it
  // has and how many its region of the traversal array has room for (equal after an upload), and where its first and last 256 positions
  // sit in key_geometry
  // ... and what yh_refit_shape needs of the shape's last BUILD (the upload or the last yh_update_shape): per width the levels of its wide
  // tree and the first node of each (wide_first[w][wide_levels[w]] = count[w]; children sit one level below their parent, so a refit
  // recomputes boxes one level per launch), and the half-area sums of the occupied slot boxes then (area_build) and now (area_now):
  // yh_shape_refit_growth is their ratio
  struct ShapeState {
    int    num_vertices, has_normals, has_texcoords, per_vertex, vert_base, elem_base, depth, depth8, depth16, count[3], room[3];
    size_t key_positions;
    int    wide_levels[3], wide_first[3][66];
    double area_build[3], area_now[3];
  };
  std::vector<ShapeState>       shape_states;
  // state
  bool             have_state = false;
  yhd_state        state{};
  yh_trace_params  params{};
  DevBuf           d_textures, d_tex_texels, d_vtex, d_maps;
  DevBuf           d_rng_state, d_rng_inc, d_accum, d_tiles, d_image, d_counters, d_tile_cursor, d_tile_cost, d_display;
  unsigned long long last_regions[3 * YH_REGIONS] = {};  // yhd_counters::region of the last yh_trace_samples_counted (yh_shade_regions)
  int              count_bound = 0;  // yh_set_count_bound: a counted launch counts the first `count_bound` items of the cost-ordered list (0: all)
  DevBuf           d_counted_items;  // ... as one byte per work item (yhd_counters::counted_items)
  std::vector<int> owned;      // owned tile ids, increasing
  std::vector<unsigned int>  item_cost;  // per work item (tile * 4 + quadrant): last measured cost (scheduling hint, kept across init_state)
  int              rank = 0, world = 1;
  int              num_tiles_total = 0;
  float            last_ms = 0;
  int              last_launches = 0;
  float            dn_ms[1 + YH_DENOISE_MAX_ITERATIONS] = {};  // yh_atrous_level_ms: the last yh_atrous_filter_gpu kernel by kernel
  int              dn_ms_count = 0;
  // the history of the temporal stage (temporal.cpp; include/yhair.h: TEMPORAL): per pixel hc = {rgb, length bits} and hg = {position, id
  // bits}, twice over — a step reads side `side` and writes the other —, the camera and the objects' frames (12 floats each, copied from
  // the object rows on the device) it was made under, and per object whether its pixels may be reused (the edits clear it, a step sets it).
  // The variance stage's moment history (include/yhair.h: VARIANCE) is a third plane beside them, hm = {M1, M2, steps bits, vt}, valid while
  // have_moments (which implies have: it lives and dies with the colour's), and d_var the variance plane of the last step that made one.
  struct Temporal {
    bool             have = false, have_moments = false;
    int              width = 0, height = 0, side = 0, num_objects = 0;
    DevBuf           hc[2], hg[2], hm[2], d_var, d_frames, d_usable;
    yh_camera        camera{};
    std::vector<int> usable;
  } tp;
  int              last_nsamples = 0;   // samples of the launch the item costs come from
  unsigned         launches_of_image = 0;  // synchronous launches since this IMAGE (scene, resolution, sampler, bounces) was first initialised: the re-planning schedule. A
                                           // re-initialised render of a known image is planned already (item_cost survives it) and goes on where the schedule was
  int              launch_shape = YH_SHAPE_QUAD;  // yhd_shape (csrc/yh_device.h: yhd_shapes), decided from launches of at least 16 spp (shorter ones have flat, noisy item costs)
  int              last_shape = -1;   // the kernel the most recent launch ran (yh_launch_shape)
  bool             async_pending = false;  // an asynchronous launch whose time yh_synchronize has still to read
  bool             last_counted = false;  // ... and whether it was the instrumented build (its time ranks nothing)
  // single-process multi-GPU gather (yh_gather_framebuffer): this context's packed tiles; on the root also the
  // receive buffer and the communicators of the device set they were made for
  DevBuf                  d_gather_send, d_gather_recv;
  std::vector<ncclComm_t> comms;
  std::vector<int>        comm_devices;
  // kernel selection by measurement (pick_launch_shape): ms per sample of a planned launch with each kernel
  // (0 = not measured yet), whether item costs exist (the first launch of a scene runs unplanned and is not a
  // measurement), and whether the scene is dense (more expensive items than resident waves; from k_trace's costs)
  double           shape_ms[YH_SHAPES] = {};   // (indexed by launch shape, yhd_state::launch_shape)
  int              shape_trials[YH_SHAPES] = {};  // trial launches behind each shape_ms (the minimum over them counts)
  uint64_t         scene_key = 0;                   // fingerprint of the uploaded scene (key of the process-wide trial record)
  bool             trials_from_disk = false;        // the record was read from the on-disk cache: complete, no trial runs
  bool             trials_on_disk = false;          // ... or has been written there by this context (once per image)
  bool             have_costs = false;
  bool             costs_settled = false;   // the item costs come from a launch of at least YH_TRIAL_SPP samples (not from the 1-spp probe)
  bool             planned_settled = false; // ... and the most recent launch was planned from such costs (only then does its time rank a kernel)
  int              dense = -1;
  int              chain16 = -1; // 1: ... and four times as many: the sixteen-lane forms are candidates too
  int              chain = -1;   // 1: so few expensive items that even twice as many waves would all be resident: the launch is bound by the
                                 // chain of steps of ONE path, and the octet kernels (half the paths per wave) are candidates
  // path pool of the streaming integrator (csrc/stream.hip): per-wave slots, allocated at its first launch
  DevBuf           d_st_slots, d_st_medium, d_st_ovf, d_st_prof, d_st_wave_log, d_st_wave_begin, d_st_wave_fill, d_scene_copy;
  int              st_items = 0;         // work items of the list k_stream's hand-out was made for (deal_items_for_stream): what its launch geometry follows
  size_t           st_share_waves = 0;   // waves the per-wave shares of the work list were made for (0: none, everything through the cursor)
  int              st_share_slots = 0;   // ... and the pool slots per wave (a share holds at most slots / 16 items)
  std::vector<int>    st_share_begin, st_share_items;  // host copy of the shares in effect: offsets per wave, items in list order
  std::vector<double> st_share_cost;                   // ... and the cost each item was planned with
  std::vector<unsigned long long> st_last_log;         // the last k_stream launch's stamps per wave {begin, end}
  bool                st_log_fresh = false;            // ... not yet used by a hand-out, and taken on the shares above
  std::vector<float>  st_wave_speed;                   // per wave of the shares' launch geometry: its speed relative to its dispatch round's (deal_shares_by_speed)
  std::vector<float>  item_scale;                      // per work item: correction of its reported cost (BVH steps) towards the time it takes (deal_shares_by_speed)
  std::vector<double> stream_speed = {1.10, 1.045, 0.97, 0.885};  // relative speed of k_stream's waves by dispatch round = hardware wave slot (prior: C2's log; every launch refines it)
  size_t           st_slots = 0, st_medium_slots = 0, st_ovf_words = 0;
  yhd_stream       stream_pool{};
};

#pragma GCC visibility push(hidden)  // internal to libyhair.so
extern std::string g_create_error;  // why yh_create returned NULL
#define HIPCHK(ctx, call)                                                                               \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(ctx, YH_E_DEVICE, "%s: %s", #call, hipGetErrorString(e_));       \
  } while (0)

// what every entry point answers on a poisoned context (wait_for_launch, trace_launch.cpp)
#define refuse_poisoned(ctx) fail(ctx, YH_E_DEVICE, "a launch of this context exceeded its deadline: the context refuses further work, destroy it")

// every wait for the context's stream is bounded (wait_for_launch, trace_launch.cpp)
#define YH_WAIT(ctx)                                      \
  do {                                                    \
    if (int wrc_ = wait_for_launch(ctx)) return wrc_;     \
  } while (0)

constexpr int YH_TRIAL_SPP = 32;  // shorter launches have flat, noisy costs: they neither rank kernels nor try new ones
constexpr double YH_TRIAL_TIE  = 1.15;
constexpr double YH_FINAL_TIE  = 1.05;  // after the trials: candidates this close to the fastest count as tied (pick_launch_shape)
constexpr int    YH_TRIALS_MAX = 2;

// ---- internal functions that cross translation units (defined in the file the comment above names) ----
int fail(yh_context* ctx, int code, const char* fmt, ...);
int upload(yh_context* ctx, DevBuf& buf, const void* src, size_t bytes);
int upload_keep(yh_context* ctx, DevBuf& buf, const void* src, size_t bytes);  // ... into a buffer that is kept while it is large enough
int alloc_zero(yh_context* ctx, DevBuf& buf, size_t bytes);
// what every sample-loop launch clears before it starts (begin_launch) and yh_init_state allocates: the cursors of the work list — one, or
// k_stream's one per item group 64 bytes apart — and a cost per work item, four items per tile
constexpr size_t YH_TILE_CURSOR_BYTES = 8 * 16 * 4;
inline size_t tile_cost_bytes(const yh_context* ctx) { return (size_t)ctx->num_tiles_total * 16; }
// entries per lane of the overflow of the lane kernels' LDS stack windows (dev_lane.h): a main ray plus a light-pdf ray above it
int lane_overflow_entries(const yh_context* ctx);
// the scene table in device memory, for the lane kernels' out-of-line callees: uploaded at the first use
int scene_copy(yh_context* ctx, const yhd_scene** sc_dev);
int dev_alloc(yh_context* ctx, DevBuf& buf, size_t bytes);  // a plain allocation: no wait, no copy, content undefined
yhd_float4 node_lo(const yhh::Node& n);
yhd_float4 node_hi(const yhh::Node& n);
void trials_load(yh_context* ctx);
bool trials_off();
void record_launch(yh_context* ctx, int nsamples, bool fresh_costs);
bool trial_pending(const yh_context* ctx);
int pick_launch_shape(const yh_context* ctx, int nsamples);
bool settle_launch_shape(yh_context* ctx, bool counted, int nsamples, bool sync);  // true: the list has to be rebuilt
void build_work_items(const yh_context* ctx, std::vector<int>& items);
void prepare_work_list(yh_context* ctx, std::vector<int>& items, int shape);
int upload_work_items(yh_context* ctx);
int expensive_items(const yh_context* ctx, const std::vector<int>& items);
bool side_by_side_grids(const yh_context* ctx, int* oct_blocks, int* quad_blocks);
void split_items_side_by_side(yh_context* ctx, std::vector<int>& items);
void lay_out_range(const yh_context* ctx, int* items, size_t n, int wpb, int G, int block_offset = 0);
int replan_after_launch(yh_context* ctx, int nsamples);
bool lane_kernels_can_address(const yh_context* ctx);  // launch_plan.cpp: the lane blob fits the one-lane kernels' 32-bit offsets
int stream_geometry(const yh_context* ctx, int num_items, int* slots_per_wave, int* grid_blocks, int* lds_out, bool* single_generation = nullptr);
void note_stream_wave_log(yh_context* ctx, const unsigned long long* log, size_t waves);
void deal_items_for_stream(yh_context* ctx, std::vector<int>& items);
int build_bvh_device(yh_context* ctx, const std::vector<yhh::Box>& boxes, yhh::Tree& tree);
int stream_impl(yh_context* ctx, int nsamples, bool sync);
// stream_report.cpp: the developer reports of a k_stream launch on stderr — YHAIR_ST_WAVELOG's, from the waves' {begin, end} stamps, and
// YHAIR_ST_PROF's, which reads the launch's counters (d_st_prof) back — and YHAIR_TIMING's stage times of one call: lap(what) prints
// "[yhair] <prefix>: <what> <ms since the last lap>", nothing when timing is off
void report_stream_waves(const yh_context* ctx, const unsigned long long* stamps, size_t waves, int waves_per_block);
int report_stream_prof(yh_context* ctx, int grid, int waves_per_block, int slots_per_wave);
struct Lap {
  const char*                           prefix;
  const bool                            on = yhh::timing();
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  explicit Lap(const char* prefix_) : prefix(prefix_) {}
  void operator()(const char* what);
};
int trace_impl(yh_context* ctx, int nsamples, bool counted, bool sync);
int wait_for_launch(yh_context* ctx);  // hipStreamSynchronize(ctx->stream) with a deadline (host/deadline.h)
int side_by_side_impl(yh_context* ctx, int nsamples, bool sync);
void destroy_communicators(yh_context* ctx);
int gbuffer_pass(yh_context* ctx, const char* who, int mode, const yh_gbuffer& planes);  // gbuffer.cpp: the feature pass into device planes (NULL: skipped), for image_pass.cpp
// denoise.cpp, for temporal.cpp: the diagonal of the uploaded scene's bounds (0 without one), and the shipped filter over a device image
// with the given device planes (those the parameters do not read may be NULL)
float scene_diagonal(const yh_context* ctx);
int denoise_with_planes(yh_context* ctx, const char* who, const yh_denoise_params& P, const void* d_in, const yh_gbuffer& guides, void* d_out);
// temporal.cpp, for the edits: the history is dropped; one object's pixels are not to be reused by the next step
void temporal_drop(yh_context* ctx);
void temporal_mark_object(yh_context* ctx, int object);
inline int tiles_of(int n) { return (n + YH_TILE - 1) / YH_TILE; }
void make_material(const yh_material& m, yhd_material& d);  // scene_upload.cpp
// scene_upload.cpp, shared with the edits: the device rows of `count` materials (`maps` / `dmaps`: theirs, or NULL in a scene without effective
// maps), true when one of them is not plain; the kernel variant and the once-per-ray form of a scene table whose materials are known; the
// fingerprint of the description the context keeps; and what a new scene does to the image state and the launch planning
bool make_material_rows(const yh_material* materials, const yh_material_maps* maps, int count, yhd_material* rows, yhd_maps* dmaps);
void settle_scene_variant(const yh_context* ctx, yhd_scene& sc, bool general_rows);
uint64_t scene_fingerprint(const yh_context* ctx);
void forget_image_of_scene(yh_context* ctx);
// scene_upload.cpp: the levels of a host-built tree as the device builder reports them (false: more than 128); the three stack needs of
// a scene (the scene level itself, shared with the edits: edit_internal.h)
// ... and shared with yh_update_shape: one shape's binary tree on the device until its collapses are made, with the index of its wide nodes;
// the upload's rule for where a shape is built; the build itself (bounds, the reference's tree, leaf-ordered records to d_recs), the
// index of its wide nodes and their collapse with the shape's test records into a traversal array
struct ShapeTree {
  int      kind = 0, num_prims = 0;
  yhh::Box root{};
  int      num_nodes = 0, levels = 1;  // the binary tree on the device: node count, levels, first node of every level
  int      level_first[130] = {0};
  int      wide_count[3] = {0, 0, 0};  // its 4- / 8- / 16-wide nodes
  int      wide_levels[3] = {1, 1, 1}, wide_first[3][66] = {};  // ... the levels of each wide tree and the first node of every level (then the count)
  int      depth = 0, depth8 = 0, depth16 = 0;  // depths of the same tree collapsed two / three / four levels at a time
  DevBuf   d_tree, d_wflag[3], d_widx[3];       // binary nodes (8 floats each); per width the flag and index of every binary node
  std::vector<yhd_float4> host_prims;  // SMALL shapes: their leaf records on the host too (the LDS light table is made from them)
};
bool shape_builds_on_device(int num_prims);
int build_shape_tree(yh_context* ctx, const char* who, int si, const yh_shape& s, bool arrays_on_device, bool on_device, yhd_float4* d_recs, ShapeTree& T);
int index_shape_tree(yh_context* ctx, const char* who, ShapeTree& T);
int collapse_shape_tree(yh_context* ctx, const char* who, const ShapeTree& T, const yh_context::LaneShape& L, void* blob);
// shape_edit.cpp: for each of `n` shapes (L[i], count[i]) per width the sum of the half-areas of the occupied slot boxes of its nodes in `blob`,
// in double and in a fixed order, to area[3 * i + w] — one allocation, 3 n kernels, one copy and one wait for all of them; what a build
// stores in ShapeState and a refit compares with
int shape_slot_areas(yh_context* ctx, const char* who, int n, const yh_context::LaneShape* L, const int (*count)[3], const void* blob, double* area);
bool tree_levels(const yhh::Tree& tree, int& levels, int* level_first);
// scene_upload.cpp, shared with the scene level of an edit: the index of the 4-wide nodes of a scene tree that is walked out of the lane
// blob — its levels, the three arrays, the nodes' copy and yhk_wide_index (which synchronises: the count comes back); `who` begins the
// message about the levels ("" for the upload)
int index_scene_tree(yh_context* ctx, const char* who, const yhh::Tree& tree, DevBuf& d_stree, DevBuf& d_sflag, DevBuf& d_sidx, int* wide_count, int* wide_depth);
struct StackNeeds { int need, need8, need16; };
// the deepest shape tree per width, over built shapes (ShapeTree) or kept ones (ShapeState); `edited`: the shape whose tree is `built` instead
struct ShapeDepths { int depth4 = 0, depth8 = 0, depth16 = 0; };
template <class Shapes>
ShapeDepths deepest_shape_trees(const Shapes& shapes, int edited = -1, const ShapeTree* built = nullptr) {
  ShapeDepths d;
  for (size_t s = 0; s < shapes.size(); s++) {
    const bool e = (int)s == edited;
    d.depth4  = std::max(d.depth4, e ? built->depth : shapes[s].depth);
    d.depth8  = std::max(d.depth8, e ? built->depth8 : shapes[s].depth8);
    d.depth16 = std::max(d.depth16, e ? built->depth16 : shapes[s].depth16);
  }
  return d;
}
#pragma GCC visibility pop
#endif
