// gbuffer.hip — the first-hit feature pass (gfx950): yh_trace_gbuffer. One lane per pixel: the camera ray (sample_camera_lane), the
// closest-hit loop of csrc/stream.hip's k_intersect_lanes (lane_step, lane_hit_retest, the exact redo of an axis-parallel ray) and the
// head of shade_step up to its YH_SHADER_NORMAL return (eval_hit, eval_hit_maps, the shading-normal rule), joined per pixel. A
// translation unit of its own, outside csrc/, so that csrc/stream.hip and the sample-loop units compile to the code they compiled to
// without it (as unit/lights_lane.hip).
//
// Why shade_step and not path_step: path_step is the product path's bounce — it reads materials from LDS, skips the maps of plain
// materials and passes through opacity. A feature buffer wants what the `normal` shader shows: the FIRST intersection, every map
// applied, rows read from memory; that is shade_step's head, and it makes the pass checkable bit for bit against that shader.
//
// Registers: __launch_bounds__(256, 3). The build comes to 140 VGPRs (144 allocated) with no vector spill and no scratch = THREE waves
// per SIMD (k_intersect_lanes: 91 registers and five). The evaluation code sits behind the traversal step and its operands are live
// across it; asked for four waves (128 registers) the build spills 4 VGPRs to scratch, so three it is. (The 86 scalar registers the
// compiler parks in VGPR lanes — the scene's and the planes' pointers — are counted in the 140.)
#define YH_LANE 1
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_path.h"

using namespace yhd;

#define YH_GB_WAVES 3         /* waves per SIMD the kernel is built for (see above) */
#define YH_GB_REFILL_LANES 16 /* idle lanes of a wave before the (divergent) refill code runs: k_intersect_lanes' figure */

// the planes of yh_gbuffer as device pointers (NULL: not asked for), and where the pixels' streams sit
struct yhk_gbuffer_args {
  int *  object, *element, *material;
  float *uv, *distance, *position, *normal, *tangent, *texcoord, *albedo, *ray;
  const uint64_t *rng_state, *rng_inc;  // YH_GBUFFER_NEXT_SAMPLE: read, never written
  int             width, height, tiles_x, mode;
};

namespace {
YH_DEV int gb_lane_rank(unsigned long long m) {  // set bits of m below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
YH_DEV void st2(float* p, size_t i, float a, float b) { p[2 * i] = a, p[2 * i + 1] = b; }
YH_DEV void st3(float* p, size_t i, f3 a) { p[3 * i] = a.x, p[3 * i + 1] = a.y, p[3 * i + 2] = a.z; }

// The planes of one finished pixel. `h` is the final hit (lane_hit_retest), (ro, rd) the ray that was traced.
YH_DEV void gb_write(const yhd_scene& sc, const yhk_gbuffer_args& g, int pixel, const hit_t& h, f3 ro, f3 rd) {
  const size_t p = (size_t)pixel;
  if (g.ray) st3(g.ray, 2 * p, ro), st3(g.ray, 2 * p + 1, rd);
  if (g.object) g.object[p] = h.object;
  if (g.uv) st2(g.uv, p, h.u, h.v);
  if (g.distance) g.distance[p] = h.distance;
  const bool geom = g.position || g.normal || g.tangent, tex = g.texcoord || g.albedo;
  if (h.object < 0) {
    if (g.element) g.element[p] = -1;
    if (g.material) g.material[p] = -1;
    if (g.position) st3(g.position, p, mk3(0.0f));
    if (g.normal) st3(g.normal, p, mk3(0.0f));
    if (g.tangent) st3(g.tangent, p, mk3(0.0f));
    if (g.texcoord) st2(g.texcoord, p, 0.0f, 0.0f);
    if (g.albedo) st3(g.albedo, p, mk3(0.0f));
    return;
  }
  if (g.element) g.element[p] = hit_element(sc, h);
  if (!g.material && !geom && !tex) return;
  const yhd_object& o = sc.objects[h.object];  // rows from memory, as shade_step reads them
  if (g.material) g.material[p] = o.material;
  if (!geom && !tex) return;
  const bool is_hair = o.kind == YH_KIND_LINES;
  float      tu = h.u, tv = h.v;
  bool       have_tc = false;
  if (geom) {
    const hit_geom hg = eval_hit(sc, o, h.slot, h.u, h.v);
    if (g.position) st3(g.position, p, hg.position);
    if (g.tangent) st3(g.tangent, p, is_hair ? hg.normal : mk3(0.0f));  // eval_normal of a line: the strand direction hair_setup takes
    if (g.normal) {
      f3             nrm = hg.normal;
      const hit_maps hm  = eval_hit_maps(sc, o, h, true, nrm);  // normal maps
      const int      thin     = sc.materials[o.material].thin;
      const f3       outgoing = -rd;
      const f3       normal   = is_hair ? quad_orthonormalize(outgoing, nrm) : ((!thin || dot(nrm, outgoing) >= 0) ? nrm : -nrm);
      st3(g.normal, p, normal);
      tu = hm.tu, tv = hm.tv, have_tc = hm.have_tc;
    }
  }
  if (tex) {
    if (!have_tc) eval_texcoord(sc, o, h, tu, tv);
    if (g.texcoord) st2(g.texcoord, p, tu, tv);
    if (g.albedo) {
      const yhd_material& mat = sc.materials[o.material];
      st3(g.albedo, p, ld3(mat.color) * eval_texture(sc, mat.color_tex, false, tu, tv));  // pt.cpp:411-412
    }
  }
}
}  // namespace

// Persistent wavefronts: LDS = the staged tables, then per wave a stack window and the cooperative line leaves' map, laid out as
// k_intersect_lanes lays them out; stack_ovf = ovf_entries x 64 entries per wave of the grid. `cursor` (zeroed by the host) deals
// the pixels in 8x8-tile order — entry k = pixel (k & 7, k >> 3 & 7) of tile k >> 6 — so that a wave's rays are neighbours.
template <int WAVES>
__global__ __launch_bounds__(256, WAVES) void k_gbuffer(const yhd_scene sc, const yhd_scene* sc_dev, const yhk_gbuffer_args g, int n,
    int* cursor, unsigned int* stack_ovf, int ovf_entries) {
  extern __shared__ v4f lds_dyn[];
  YH_LDS v4f* lds_tabs = (YH_LDS v4f*)lds_dyn;
  const int   lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  YH_LDS unsigned int* w_stack = (YH_LDS unsigned int*)(lds_tabs + YHD_LDS_TABLES_F4(&sc)) + wib * (64 * YH_LSTACK + 128);
  YH_LDS unsigned long long* w_cmap = (YH_LDS unsigned long long*)(size_t)__builtin_amdgcn_readfirstlane((unsigned int)(size_t)(w_stack + 64 * YH_LSTACK));
  trace_ctx tc;
  tc.sc = &sc, tc.sc_dev = sc_dev, tc.lds_stack = nullptr, tc.stats = nullptr;
  YH_LDS float* lds_cam;
  stage_tables(sc, lds_tabs, threadIdx.x, 256, tc, lds_cam);
  __syncthreads();
  const size_t wave_id = (size_t)blockIdx.x * 4 + wib;
  lane_stack   stk;
  stk.lds = w_stack + lane, stk.ovf = stack_ovf + wave_id * (size_t)ovf_entries * 64 + lane, stk.sp = 0, stk.base = 0;
  tc.ls = &stk;
  lane_trav t;
  lane_begin(sc, t, mk3(0.0f), mk3(1.0f), -1);
  bool have = false, dry = false;
  int  pixel = 0;
  while (true) {
    const unsigned long long idle  = __ballot(!have);
    const int                nidle = (int)__popcll(idle);
    if (!dry && (nidle >= YH_GB_REFILL_LANES || nidle == 64)) {
      int first = 0;
      if (lane == 0) first = atomicAdd(cursor, nidle);
      first = __builtin_amdgcn_readfirstlane(first);
      if (first >= n) dry = true;
      const int mine = first + gb_lane_rank(idle);
      if (!have && mine < n) {
        const int tile = mine >> 6, i = (tile % g.tiles_x) * YH_TILE + (mine & 7), j = (tile / g.tiles_x) * YH_TILE + ((mine >> 3) & 7);
        if (i < g.width && j < g.height) {  // (an edge tile's entries outside the image stay idle)
          pixel = j * g.width + i;
          float lu = 0.0f, lv = 0.0f, pu = 0.5f, pv = 0.5f;
          yhd_camera cam;
          for (int k = 0; k < 12; k++) cam.frame[k] = lds_cam[k];
          cam.lens = lds_cam[12], cam.film_x = lds_cam[13], cam.film_y = lds_cam[14], cam.focus = lds_cam[15], cam.aperture = lds_cam[16];
          if (g.mode == YH_GBUFFER_NEXT_SAMPLE) {  // the draws of path_begin on a copy of the pixel's stream: nothing is written back
            rng_t rng;
            rng.state = g.rng_state[pixel], rng.inc = g.rng_inc[pixel];
            lu = rand1f(rng), lv = rand1f(rng);
            pu = rand1f(rng), pv = rand1f(rng);
          } else {
            cam.aperture = 0.0f;  // the pinhole ray through the pixel centre whatever the lens
          }
          const ray_t r = sample_camera_lane(cam, i, j, g.width, g.height, pu, pv, lu, lv);
          lane_begin(sc, t, r.o, r.d, -1);
          have = true;
        }
      }
    }
    if (__ballot(have) == 0) {
      if (dry) break;
      continue;
    }
    bool redo = false;
    if (lane_step<false, false, true, true>(tc, t, stk, 0, redo, nullptr, have, w_cmap)) {
      have    = false;
      hit_t h = lane_hit_retest(tc, t.hit, t.hit_lines, t.ro, t.rd);
      if (redo) {  // axis-parallel ray: the reference's compare-and-select box test throughout
        stk.sp = 0, stk.base = 0;
        lane_exact_result e = sc.scene_wide_root >= 0 ? lane_trace_exact_wide(sc_dev, tc.lds_scene, stk.lds, stk.ovf, 0, 0, t.ro, t.rd, -1)
                                                      : lane_trace_exact(sc_dev, tc.lds_scene, stk.lds, stk.ovf, 0, 0, t.ro, t.rd, -1);
        stk.base = e.base;
        h        = lane_hit_retest(tc, e.hit, e.hit_lines != 0, t.ro, t.rd);
      }
      gb_write(sc, g, pixel, h, t.ro, t.rd);
    }
  }
}

extern "C" {
typedef void (*gbuffer_kernel_t)(const yhd_scene, const yhd_scene*, const yhk_gbuffer_args, int, int*, unsigned int*, int);
static gbuffer_kernel_t gbuffer_kernel() { return k_gbuffer<YH_GB_WAVES>; }
int yhk_gbuffer_waves(void) { return YH_GB_WAVES; }
static int gbuffer_lds(const yhd_scene* sc) { return YHD_LDS_TABLES_F4(sc) * 16 + 4 * (64 * YH_LSTACK * 4 + 64 * 8); }
// resident 256-thread workgroups per CU with the scene's LDS layout (0: the kernel cannot run)
int yhk_gbuffer_occupancy(const yhd_scene* sc) {
  int blocks = 0, lds = gbuffer_lds(sc);
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)gbuffer_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, gbuffer_kernel(), 256, lds) != hipSuccess) return 0;
  return blocks;
}
// planes: the eleven pointers of yh_gbuffer in its order, device memory; cursor: one zeroed int; stack_ovf: ovf_entries x 64 entries for each
// of the grid's grid_blocks x 4 waves
int yhk_gbuffer(const yhd_scene* sc, const yhd_scene* sc_dev, const yhd_state* st, int mode, void* const planes[11], int* cursor,
    unsigned int* stack_ovf, int ovf_entries, int grid_blocks, hipStream_t stream) {
  yhk_gbuffer_args g;
  g.object = (int*)planes[0], g.element = (int*)planes[1], g.material = (int*)planes[2];
  g.uv = (float*)planes[3], g.distance = (float*)planes[4], g.position = (float*)planes[5], g.normal = (float*)planes[6];
  g.tangent = (float*)planes[7], g.texcoord = (float*)planes[8], g.albedo = (float*)planes[9], g.ray = (float*)planes[10];
  g.rng_state = st->rng_state, g.rng_inc = st->rng_inc;
  g.width = st->width, g.height = st->height, g.tiles_x = (st->width + YH_TILE - 1) / YH_TILE, g.mode = mode;
  const int n   = g.tiles_x * ((st->height + YH_TILE - 1) / YH_TILE) * 64;
  const int lds = gbuffer_lds(sc);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)gbuffer_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(gbuffer_kernel(), dim3(grid_blocks), dim3(256), lds, stream, *sc, sc_dev, g, n, cursor, stack_ovf, ovf_entries);
  return (int)hipGetLastError();
}
}
