// kernels.hip — the quad sample-loop kernels (gfx950) and nothing else: their instantiations, the choice among them and their launch.
//
//   k_trace          the sample loop (trace_samples, pt.cpp:1992-2007) with a QUAD per path: persistent
//                    wavefronts pull 4x4-pixel work items (most expensive first); four adjacent lanes own one
//                    pixel / one path (its PCG32 stream is sequential) and split BVH steps and hair lobes over
//                    their lanes. In LDS: the traversal stacks (one column per quad, sized by the scene's
//                    need) and the tables of dev_trace.h: stage_tables — scene level, camera, small area
//                    lights, the index of the environment cdf, the material table. Two launch shapes: 512 threads
//                    x 4 waves per SIMD, 256 x 5. The other sample-loop kernels: csrc/wide.hip (more lanes per
//                    path), csrc/stream.hip (k_stream, one lane per path); the host picks per launch by measurement.
//   k_trace_shader   the same loop for the preview shaders (naive, eyelight, normal), at the 512 x 4 shape
//   trace_kernel     which instantiation a launch runs; trace_lds: its dynamic LDS; yhk_trace: the launch, and the small queries the
//                    host plans with (yhk_block_threads, yhk_stack_entries, yhk_trace_lds_bytes, yhk_trace_occupancy)
//
// Every other kernel — the unit-level batches, the self-tests, the framebuffer kernels — lives in unit/, a file per subject with its
// launchers, so that an edit there neither recompiles this translation unit nor changes the code of its loops.
// Compiled with -ffp-contract=off (see dev_math.h).
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "launchers.h"
#include "dev_items.h"

template <int SHADER>
__global__ __launch_bounds__(YH_BLOCK, YH_MIN_WAVES) void k_trace_shader(const yhd_scene sc, const yhd_state st,
    int nsamples, yhd_counters* counters) {
  trace_items<false, true, YH_BLOCK, SHADER>(sc, st, nsamples, counters);
}

extern "C" {

#define YH_DENSE_WAVES 5 /* 96 VGPRs: at 6 (80 VGPRs) the traversal loop itself spills and the kernel is at the mercy of the register allocator (measured 0.6-0.75x after an unrelated change of the shading code, profiles/r02) */
// The k_trace launch shapes (csrc/yh_device.h: yhd_shapes): quads over 4-wide nodes at 512 x 4 and at 256 x YH_DENSE_WAVES, and the wide forms
static_assert(yhd_shapes[YH_SHAPE_QUAD].block_threads == YH_BLOCK && yhd_shapes[YH_SHAPE_OCT].block_threads == YH_OCT_BLOCK && yhd_shapes[YH_SHAPE_HEX].block_threads == YH_OCT_BLOCK, "yhd_shapes");
static int shape_block(int shape) { return yhd_shapes[shape].block_threads; }
static int shape_groups(int shape) { return shape_block(shape) / yhd_shapes[shape].lanes_per_path; }
// `once`: the scene takes the form that resolves the scene level once per ray (yhd_scene::scene_once): shape 0's plain variants have it
// `cenv`: ... and its lights are constant environments (yhd_scene::lights_const_env): shape 0's plain variants have a form for that too
static trace_kernel_t trace_kernel(bool counted, bool general, int shape, int shader = YH_SHADER_PATH, bool once = false, bool cenv = false) {
  if (shader == YH_SHADER_NAIVE) return k_trace_shader<YH_SHADER_NAIVE>;
  if (shader == YH_SHADER_EYELIGHT) return k_trace_shader<YH_SHADER_EYELIGHT>;
  if (shader == YH_SHADER_NORMAL) return k_trace_shader<YH_SHADER_NORMAL>;
  if (yhd_shapes[shape].kind == YH_SHAPE_KIND_WIDE) return yhk_wide_kernel(counted ? 1 : 0, general ? 1 : 0, shape);  // csrc/wide.hip
  if (yhd_shapes[shape].kind == YH_SHAPE_KIND_RETIRED) return nullptr;
  // The GENERAL variants carry the surface lobes, volumes, textures and the through-memory light code. The dense shape
  // spilled 184 registers at the plain variant's 96 (7 scratch instructions inside its traversal loops): it runs at 256 x 4
  // (128 registers, 49 spilled, none in the traversal loops; lobes / volumes +15-20 %, profiles/r03/general_waves_ab.txt).
  // The 512-thread shape stays at 4 waves per SIMD (68 spilled, none in the traversal loops): at 3 (168 registers, 2
  // spilled) its expensive items no longer fit the resident waves and it loses a third.
  if (general && !counted && shape == YH_SHAPE_QUAD_DENSE) return k_trace<false, true, 256, YH_DENSE_WAVES - 1>;
  if (shape == YH_SHAPE_QUAD_DENSE)
    return counted ? (general ? k_trace<true, true, 256, YH_DENSE_WAVES> : k_trace<true, false, 256, YH_DENSE_WAVES>)
                   : (general ? k_trace<false, true, 256, YH_DENSE_WAVES> : k_trace<false, false, 256, YH_DENSE_WAVES>);
  if (cenv && !general)
    return counted ? (once ? k_trace_cenv<true, true> : k_trace_cenv<true, false>) : (once ? k_trace_cenv<false, true> : k_trace_cenv<false, false>);
  if (once && !general) return counted ? k_trace<true, false, YH_BLOCK, YH_MIN_WAVES, YH_MODE_QUAD, true> : k_trace<false, false, YH_BLOCK, YH_MIN_WAVES, YH_MODE_QUAD, true>;
  return counted ? (general ? k_trace<true, true, YH_BLOCK, YH_MIN_WAVES> : k_trace<true, false, YH_BLOCK, YH_MIN_WAVES>)
                 : (general ? k_trace<false, true, YH_BLOCK, YH_MIN_WAVES> : k_trace<false, false, YH_BLOCK, YH_MIN_WAVES>);
}
static size_t trace_lds(const yhd_scene* sc, int shape) {
  const int lanes   = yhd_shapes[shape].lanes_per_path;
  const int entries = lanes == 16 ? sc->stack_entries16 : lanes == 8 ? sc->stack_entries8 : sc->stack_entries;
  // (the records of the ONCE form behind the tables: shape 0 — its plain variants read them; k_trace_exact and the preview shaders,
  // which launch with this geometry, leave them unused)
  const size_t once = shape == YH_SHAPE_QUAD ? (size_t)YHD_ONCE_F4(sc, shape_groups(shape)) * 16 : 0;
  return (size_t)(entries + YH_HITROWS) * shape_groups(shape) * 4 + (size_t)YHD_LDS_TABLES_F4(sc) * 16 + once;
}
// `shape`: a k_trace one (quad or wide); the caller built the work list for it (yhd_shape_info::entries_per_item)
int yhk_trace(const yhd_scene* sc, const yhd_state* st, int nsamples, yhd_counters* counters, int shape,
    int grid_blocks, hipStream_t stream) {
  const bool path  = st->shader == YH_SHADER_PATH;
  if (!path) shape = YH_SHAPE_QUAD;  // the other shaders have one shape (512 x 4)
  if (!path && counters) return (int)hipErrorInvalidValue;
  if ((unsigned)shape >= YH_SHAPES || yhd_shapes[shape].kind == YH_SHAPE_KIND_STREAM || yhd_shapes[shape].kind == YH_SHAPE_KIND_SBS) return (int)hipErrorInvalidValue;
  size_t    lds   = trace_lds(sc, shape);
  trace_kernel_t k     = trace_kernel(counters != nullptr, sc->general_materials != 0, shape, st->shader, sc->scene_once > 0, sc->lights_const_env != 0);
  if (!k) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {  // above 64 KB the dynamic-LDS limit must be raised explicitly; the attribute is per
                          // device, so it is set for the current device at every such launch (no process-wide cache)
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k, dim3(grid_blocks), dim3(shape_block(shape)), lds, stream, *sc, *st, nsamples, counters);
  return (int)hipGetLastError();
}
int yhk_block_threads(int shape) { return shape_block(shape); }
int yhk_stack_entries(void) { return YH_QSTACK; }
int yhk_trace_lds_bytes(const yhd_scene* sc, int shape) { return (int)trace_lds(sc, shape); }
// (asked of the variant without the ONCE form: the two have one launch bound and differ in nothing the answer depends on but
// `lds_bytes`, which the caller gives)
int yhk_trace_occupancy(int lds_bytes, int general, int shape) {
  int            blocks = 0;
  trace_kernel_t k      = trace_kernel(false, general != 0, shape);
  if (!k) return 0;  // a launch shape this build does not contain
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess)
    return 0;  // the kernel cannot be launched with this much LDS: the caller reports it
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, shape_block(shape), lds_bytes) != hipSuccess) return 1;
  return blocks < 1 ? 0 : blocks;
}
}
