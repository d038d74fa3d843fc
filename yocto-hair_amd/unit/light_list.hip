// light_list.hip — the light list of an uploaded scene made again where its data is (yh_set_light_edits: an edit that turns a light on or
// off or reshapes an emitter; yh_triangle_cdf_gpu), init_lights' rule (pt.cpp:1695-1740) as the upload runs it on the host:
//   k_light_cdf       the area cdf of every area light of the new list, one WAVE (a workgroup of 64) per light, several lights per launch.
//                     The entries are cdf[t] = area[t] + cdf[t - 1] as ONE float chain in element order — float addition is not
//                     associative, so a tree scan, a pairwise sum or per-block partial sums give other bits than the upload's loop. The
//                     wave loads 64 triangles at a time (coalesced rows of elems, then vpos) and computes their areas in parallel
//                     (unit/light_math.h, the text the upload compiles); the additions then run lane by lane in registers: every lane
//                     reads lane l's area (v_readlane, a scalar), adds it to the running sum all lanes carry alike, and lane l keeps the
//                     sum at its turn. Nothing passes between workgroups: a light's chain lives in its own wave, no flags, no waiting.
//   k_small_records   per small light (at most YH_SMALL_LIGHT_TRIS triangles) its record of the kernels' LDS light table (yh_device.h): the
//                     shape's root box, the count, the total area, the triangles in LEAF order from the shape's records, the cdf by element;
//   k_env_tab         the coarse index of one environment light's texel cdf: tab[k] = cdf[min(n, (k + 1) S) - 1].
// An environment's texel cdf is NOT made here: the upload computes it with the host's sine, whose last place the device's does not share.
// A translation unit of its own: the sample-loop units do not see it. Not a hot path in the kernels' sense: no LDS, plain C++.
#include <hip/hip_runtime.h>

#include "../csrc/yh_device.h"
#include "../csrc/launchers.h"
#include "light_list.h"
#include "light_math.h"

namespace {

// raw: the unit-level form, positions as 3 floats per vertex and triangles as 3 ints (pos, tri); else the scene's rows (vpos, elems)
__global__ __launch_bounds__(64) void k_light_cdf(const yhk_light_job* jobs, const float4* vpos, const int4* elems, const float* pos, const int* tri, float* cdf) {
  const yhk_light_job J    = jobs[blockIdx.x];
  const int           lane = (int)threadIdx.x;
  float               run  = 0;  // (the first entry is its area: 0 + a is a for an area, which is never -0)
  for (int base = 0; base < J.count; base += 64) {
    const int t    = base + lane;
    float     area = 0;
    if (t < J.count) {
      F3 p0, p1, p2;
      if (pos) {
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        p0 = ld3(pos + 3 * (size_t)a), p1 = ld3(pos + 3 * (size_t)b), p2 = ld3(pos + 3 * (size_t)c);
      } else {
        const int4   e = elems[(size_t)J.elem_base + t];
        const float4 a = vpos[(size_t)J.vert_base + e.x], b = vpos[(size_t)J.vert_base + e.y], c = vpos[(size_t)J.vert_base + e.z];
        p0 = {a.x, a.y, a.z}, p1 = {b.x, b.y, b.z}, p2 = {c.x, c.y, c.z};
      }
      area = triangle_area(p0, p1, p2);
    }
    float mine = 0;
#pragma unroll
    for (int l = 0; l < 64; l++) {  // the chain: 64 dependent additions, the same in every lane (lanes behind the end add 0 after the last entry)
      run = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(area), l)) + run;
      if (lane == l) mine = run;
    }
    if (t < J.count) cdf[(size_t)J.cdf_base + t] = mine;
  }
}

__global__ void k_small_records(int num_jobs, const yhk_light_job* jobs, const float* root6, const float4* prims, const float* cdf, float4* table) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= num_jobs) return;
  const yhk_light_job J = jobs[i];
  if (J.small_base < 0) return;
  const float*  b   = root6 + 6 * (size_t)J.shape;
  const float4* rec = prims + J.prim_base;
  float4*       out = table + J.small_base;
  out[0] = {b[0], b[1], b[2], __int_as_float(J.count)};
  out[1] = {b[3], b[4], b[5], cdf[(size_t)J.cdf_base + J.count - 1]};
  for (int t = 0; t < YH_SMALL_LIGHT_TRIS; t++)
    for (int k = 0; k < 3; k++) out[2 + 3 * t + k] = t < J.count ? rec[6 * t + k] : float4{0, 0, 0, 0};
  float c[4] = {0, 0, 0, 0};
  for (int t = 0; t < J.count && t < YH_SMALL_LIGHT_TRIS; t++) c[t] = cdf[(size_t)J.cdf_base + t];
  out[2 + 3 * YH_SMALL_LIGHT_TRIS] = {c[0], c[1], c[2], c[3]};
}

__global__ void k_env_tab(int K, int S, int n, const float* cdf, float* tab) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= K) return;
  const long long end = (long long)(k + 1) * S;
  tab[k] = cdf[(size_t)(end < n ? end : n) - 1];
}

}  // namespace

static_assert(sizeof(yhk_light_job) == 32, "jobs are copied to the device as they are");
static_assert(YH_SMALL_LIGHT_F4 == 3 + 3 * YH_SMALL_LIGHT_TRIS && YH_SMALL_LIGHT_TRIS == 4, "the cdf of a small light is one float4");

extern "C" int yhk_light_cdfs(int num_jobs, const void* jobs, const void* vpos, const void* elems, float* cdf, hipStream_t stream) {
  if (num_jobs <= 0) return 0;
  hipLaunchKernelGGL(k_light_cdf, dim3((unsigned)num_jobs), dim3(64), 0, stream, (const yhk_light_job*)jobs, (const float4*)vpos, (const int4*)elems, (const float*)nullptr,
      (const int*)nullptr, cdf);
  return (int)hipGetLastError();
}

extern "C" int yhk_triangle_cdf_raw(const void* job, const float* pos, const int* tri, float* cdf, hipStream_t stream) {
  hipLaunchKernelGGL(k_light_cdf, dim3(1), dim3(64), 0, stream, (const yhk_light_job*)job, (const float4*)nullptr, (const int4*)nullptr, pos, tri, cdf);
  return (int)hipGetLastError();
}

extern "C" int yhk_small_records(int num_jobs, const void* jobs, const float* root6, const void* prims, const float* cdf, void* table, hipStream_t stream) {
  if (num_jobs <= 0) return 0;
  hipLaunchKernelGGL(k_small_records, dim3(1), dim3(64), 0, stream, num_jobs, (const yhk_light_job*)jobs, root6, (const float4*)prims, cdf, (float4*)table);
  return (int)hipGetLastError();
}

extern "C" int yhk_env_tab(int K, int S, int n, const float* cdf, float* tab, hipStream_t stream) {
  if (K <= 0) return 0;
  hipLaunchKernelGGL(k_env_tab, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, K, S, n, cdf, tab);
  return (int)hipGetLastError();
}
