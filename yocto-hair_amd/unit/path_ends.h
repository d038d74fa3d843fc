// path_ends.h — the body of the unit-level kernels of the code that starts and ends a path (yh_path_ends_batch): path_begin with
// sample_camera / sample_camera_lane, path_continue and path_end of dev_path.h, row by row. Every step calls the device functions of
// dev_path.h / dev_trace.h themselves; the one restatement is the four rand1f draws in front of sample_camera_lane, written as the finish
// stage of csrc/stream.hip and unit/gbuffer.hip write them (tests/test_path_ends.py ties them to the feature pass bit for bit).
//
// Compiled twice, as the sample loop is: unit/path_ends_quad.hip (a quad per row, as the quad loops of csrc/dev_items.h run them: the four
// lanes of a quad with identical arguments) and unit/path_ends_lane.hip with YH_LANE 1 (a lane per row, as k_stream runs them).
//
// Per row and operation (include/yhair.h: YH_PATH_*):
//   begin     fin 17 = yhd_camera, iin 4 = i, j, w, h, rng 2 = state, inc
//             quad: path_begin(cam, ps, rng, i, j, w, h); lane: lu, lv, pu, pv = rand1f(rng) x 4, sample_camera_lane(cam, ...)
//             fout 12 = ray.o[3], ray.d[3], radiance[3], weight[3]; iout 3 = bounce, hit, in_medium (lane: the ray, the rest zero); state
//   continue  fin 3 = weight, iin 2 = bounce, bounces, rng 2
//             path_continue(ps, rng, bounces); fout 3 = weight; iout 2 = the flag, bounce; state
//   end       fin 8 = radiance[3], clamp, acc[4], iin 1 = hit
//             path_end(ps, clamp, acc); fout 4 = acc
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "dev_path.h"

using namespace yhd;

YH_DEV void path_ends_row(int op, const float* fi, const int* ii, const uint64_t* rs, bool write, float* fo, int* io, uint64_t* so) {
  path_t ps;
  ps.radiance = mk3(0.0f), ps.weight = mk3(0.0f), ps.bounce = 0, ps.hit = false, ps.in_medium = false;
#if YH_LANE
  ps.medium_mem = nullptr;
#endif
  if (op == YH_PATH_BEGIN) {
    const yhd_camera& cam = *(const yhd_camera*)fi;
    rng_t rng{rs[0], rs[1]};
#if YH_LANE
    float lu = rand1f(rng), lv = rand1f(rng);
    float pu = rand1f(rng), pv = rand1f(rng);
    ps.ray = sample_camera_lane(cam, ii[0], ii[1], ii[2], ii[3], pu, pv, lu, lv);
#else
    path_begin(cam, ps, rng, ii[0], ii[1], ii[2], ii[3]);
#endif
    if (!write) return;
    fo[0] = ps.ray.o.x, fo[1] = ps.ray.o.y, fo[2] = ps.ray.o.z, fo[3] = ps.ray.d.x, fo[4] = ps.ray.d.y, fo[5] = ps.ray.d.z;
    fo[6] = ps.radiance.x, fo[7] = ps.radiance.y, fo[8] = ps.radiance.z, fo[9] = ps.weight.x, fo[10] = ps.weight.y, fo[11] = ps.weight.z;
    io[0] = ps.bounce, io[1] = ps.hit ? 1 : 0, io[2] = ps.in_medium ? 1 : 0;
    so[0] = rng.state;
  } else if (op == YH_PATH_CONTINUE) {
    rng_t rng{rs[0], rs[1]};
    ps.weight = ld3(fi), ps.bounce = ii[0];
    const bool goes_on = path_continue(ps, rng, ii[1]);
    if (!write) return;
    fo[0] = ps.weight.x, fo[1] = ps.weight.y, fo[2] = ps.weight.z;
    io[0] = goes_on ? 1 : 0, io[1] = ps.bounce;
    so[0] = rng.state;
  } else {
    ps.radiance = ld3(fi), ps.hit = ii[0] != 0;
    yhd_float4 acc = {fi[4], fi[5], fi[6], fi[7]};
    path_end(ps, fi[3], acc);
    if (!write) return;
    fo[0] = acc.x, fo[1] = acc.y, fo[2] = acc.z, fo[3] = acc.w;
  }
}

// nfi, nii, nfo, nio: the floats / ints per row of the operation (yhk_path_ends_* below); rng 2 per row, state 1 per row (not `end`)
__global__ __launch_bounds__(256) void YH_PATH_ENDS_KERNEL(int op, int n, int nfi, int nii, int nfo, int nio, const float* fin, const int* iin,
    const uint64_t* rng, float* fout, int* iout, uint64_t* state) {
  constexpr bool QUAD = !YH_LANE;
  int  i     = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> (QUAD ? 2 : 0);
  bool valid = i < n;
  if (!valid) {
    if (!QUAD) return;
    i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  }
  const size_t r = (size_t)i;
  path_ends_row(op, fin + nfi * r, iin + nii * r, rng + 2 * r, valid && (!QUAD || (threadIdx.x & 3) == 0), fout + nfo * r, iout + nio * r, state + r);
}

extern "C" int YH_PATH_ENDS_LAUNCH(int op, int n, const float* fin, const int* iin, const uint64_t* rng, float* fout, int* iout, uint64_t* state,
    hipStream_t s) {
  if (n < 1 || op < 0 || op >= YH_PATH_OPS) return (int)hipErrorInvalidValue;
  static const int floats_in[YH_PATH_OPS] = {YH_PATH_BEGIN_IN, YH_PATH_CONTINUE_IN, YH_PATH_END_IN}, ints_in[YH_PATH_OPS] = {4, 2, 1};
  static const int floats_out[YH_PATH_OPS] = {YH_PATH_BEGIN_OUT, YH_PATH_CONTINUE_OUT, YH_PATH_END_OUT}, ints_out[YH_PATH_OPS] = {3, 2, 0};
  const int rows_per_block = YH_LANE ? 256 : 64;
  hipLaunchKernelGGL(YH_PATH_ENDS_KERNEL, dim3((n + rows_per_block - 1) / rows_per_block), dim3(256), 0, s, op, n, floats_in[op], ints_in[op],
      floats_out[op], ints_out[op], fin, iin, rng, fout, iout, state);
  return (int)hipGetLastError();
}
