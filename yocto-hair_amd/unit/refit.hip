// refit.hip — yh_refit_shape / yh_refit_shape_device / yh_bvh_refit_wide_gpu: a shape's tree keeps its topology, its primitives are
// written again in their leaf slots and the boxes of its 4- / 8- / 16-wide nodes are recomputed bottom-up, in place:
//   k_refit_boxes        per leaf slot the line_bounds / triangle_bounds of the element its record holds, from the new arrays (24 bytes per
//                        primitive, LEAF order: what the leaves of all three widths read). Writes nothing of the scene: it runs before the
//                        edit can still refuse;
//   k_box_partials       the union of those boxes per block (the shape's new root box: min / max are exact, the host unites the partials);
//   k_refit_records      per leaf slot the record again, the bits k_leaf_records (csrc/bvh_gpu.hip) writes for that element;
//   k_refit_wide<L>      one thread per wide node of ONE LEVEL of the wide tree, deepest level first, one launch per level: a leaf slot's box
//                        from the primitive boxes, an internal slot's from the slots of the child node it refers to — which the launch before
//                        wrote. No thread reads what its own launch writes (a node's children sit one level down), so nothing is handed from
//                        workgroup to workgroup inside a launch: no flags, no counters, no waiting, and the launch boundary orders the levels.
//                        ref, axes and the occupied bits are not written: a float4 and a float2 store per slot;
//   k_area_partials      the half-areas of a width's occupied slot boxes, summed in double in a fixed order (yh_shape_refit_growth).
// The unions nest as the binary tree's do (a slot index is the path below the wide node's root, so siblings are neighbours): the boxes
// are the bits a build over the same leaf order forms, signed zeros included. Not a hot path in the kernels' sense: no LDS but the
// block reductions', plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "launchers.h"

namespace {

__device__ __forceinline__ float fmin_(float a, float b) { return (a < b) ? a : b; }  // math.h:1779
__device__ __forceinline__ float fmax_(float a, float b) { return (a > b) ? a : b; }

struct Box6 {
  float mn[3], mx[3];
};
__device__ __forceinline__ Box6 unite(const Box6& a, const Box6& b) {  // (a first: what k_boxes / build_bvh do with a node's two children)
  Box6 r;
  for (int k = 0; k < 3; k++) r.mn[k] = fmin_(a.mn[k], b.mn[k]), r.mx[k] = fmax_(a.mx[k], b.mx[k]);
  return r;
}

// the element id a leaf record holds (yh_device.h: a segment keeps it in {t0, element}, a triangle in {p0, element})
__device__ __forceinline__ int record_element(int lines, const float4* recs, size_t slot) {
  return __float_as_int(lines ? recs[4 * slot + 2].w : recs[6 * slot].w);
}

// line_bounds / triangle_bounds (math.h:3037-3044), radius 0.001 when the shape has none: k_prim_boxes' arithmetic, in leaf order
__global__ void k_refit_boxes(int lines, int n, const float4* recs, const float* pos, const float* radius, const int* idx, float* boxes) {
  const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (size_t)n) return;
  const size_t e = (size_t)record_element(lines, recs, slot);
  float*       o = boxes + 6 * slot;
  if (lines) {
    int   a = idx[2 * e], b = idx[2 * e + 1];
    float r0 = radius ? radius[a] : 0.001f, r1 = radius ? radius[b] : 0.001f;
    for (int k = 0; k < 3; k++) {
      float p0 = pos[3 * (size_t)a + k], p1 = pos[3 * (size_t)b + k];
      o[k] = fmin_(p0 - r0, p1 - r1), o[3 + k] = fmax_(p0 + r0, p1 + r1);
    }
  } else {
    const float* p0 = pos + 3 * (size_t)idx[3 * e];
    const float* p1 = pos + 3 * (size_t)idx[3 * e + 1];
    const float* p2 = pos + 3 * (size_t)idx[3 * e + 2];
    for (int k = 0; k < 3; k++) o[k] = fmin_(p0[k], fmin_(p1[k], p2[k])), o[3 + k] = fmax_(p0[k], fmax_(p1[k], p2[k]));
  }
}

constexpr int RB = 256;  // threads of the two reductions

// partial[block] = the union of boxes[i], i = block * RB + thread + j * grid * RB (a strided share, then the block's tree)
__global__ void k_box_partials(int n, const float* boxes, float* partial) {
  __shared__ float sh[RB][6];
  const float      inf = __int_as_float(0x7f800000);
  float            b[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (size_t i = (size_t)blockIdx.x * RB + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * RB)
    for (int k = 0; k < 3; k++) b[k] = fmin_(b[k], boxes[6 * i + k]), b[3 + k] = fmax_(b[3 + k], boxes[6 * i + 3 + k]);
  for (int k = 0; k < 6; k++) sh[threadIdx.x][k] = b[k];
  __syncthreads();
  for (int half = RB / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      for (int k = 0; k < 3; k++) {
        sh[threadIdx.x][k]     = fmin_(sh[threadIdx.x][k], sh[threadIdx.x + half][k]);
        sh[threadIdx.x][3 + k] = fmax_(sh[threadIdx.x][3 + k], sh[threadIdx.x + half][3 + k]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) partial[6 * (size_t)blockIdx.x + threadIdx.x] = sh[0][threadIdx.x];
}

// the record of leaf slot `slot` again, in place: k_leaf_records with the element read from the record instead of the leaf order
__global__ void k_refit_records(int lines, int n, const float* pos, const float* nrm, const float* radius, const int* idx, float4* recs) {
  const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (size_t)n) return;
  const int   e  = record_element(lines, recs, slot);
  const float ew = __int_as_float(e);
  auto P = [&](int v) { return make_float3(pos[3 * (size_t)v], pos[3 * (size_t)v + 1], pos[3 * (size_t)v + 2]); };
  auto N = [&](int v) { return nrm ? make_float3(nrm[3 * (size_t)v], nrm[3 * (size_t)v + 1], nrm[3 * (size_t)v + 2]) : make_float3(0, 0, 0); };
  if (lines) {
    int     a = idx[2 * (size_t)e], b = idx[2 * (size_t)e + 1];
    float3  p0 = P(a), p1 = P(b), t0 = N(a), t1 = N(b);
    float4* r = recs + 4 * slot;
    r[0] = make_float4(p0.x, p0.y, p0.z, radius ? radius[a] : 0.001f), r[1] = make_float4(p1.x, p1.y, p1.z, radius ? radius[b] : 0.001f);
    r[2] = make_float4(t0.x, t0.y, t0.z, ew), r[3] = make_float4(t1.x, t1.y, t1.z, 0.0f);
  } else {
    int     a = idx[3 * (size_t)e], b = idx[3 * (size_t)e + 1], c = idx[3 * (size_t)e + 2];
    float3  p0 = P(a), p1 = P(b), p2 = P(c), n0 = N(a), n1 = N(b), n2 = N(c);
    float4* r = recs + 6 * slot;
    r[0] = make_float4(p0.x, p0.y, p0.z, ew), r[1] = make_float4(p1.x, p1.y, p1.z, 0.0f), r[2] = make_float4(p2.x, p2.y, p2.z, 0.0f);
    r[3] = make_float4(n0.x, n0.y, n0.z, 0.0f), r[4] = make_float4(n1.x, n1.y, n1.z, 0.0f), r[5] = make_float4(n2.x, n2.y, n2.z, 0.0f);
  }
}

// Wide nodes [first, first + count) of one level. blob: the slot array, 32-byte units {min.xyz, max.x}{max.yz, ref, axes}; node i of the
// shape begins at unit node_off + W * i; a leaf's reference holds test_off + units * (its first leaf slot) in the low 27 bits and its count
// in bits 27-29; lboxes: the primitive boxes in leaf order (a leaf's range lies inside them: the context wrote the reference itself, and
// the unit entry checks every leaf before it launches, yhh::wide_levels). Two float4 loads per slot read, 16 bytes each.
template <int L>
__global__ void k_refit_wide(float4* blob, unsigned int node_off, int first, int count, unsigned int test_off, unsigned int units, const float* lboxes) {
  constexpr int W = 1 << L;
  const int     t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const float inf = __int_as_float(0x7f800000);
  float4*     node = blob + 2 * ((size_t)node_off + (size_t)W * (size_t)(first + t));
  for (int s = 0; s < W; s++) {
    const float4   hi  = node[2 * s + 1];
    const unsigned ref = __float_as_uint(hi.z);
    if (ref == 0xFFFFFFFFu) continue;  // an empty slot keeps +-inf
    Box6 box;
    if (ref & 0x80000000u) {  // a leaf: its primitives in leaf order, from FLT_MAX as the builders start (k_boxes, build_bvh)
      const int      num   = (int)((ref >> 27) & 7u);
      const unsigned start = ((ref & 0x07FFFFFFu) - test_off) / units, end = start + (unsigned)num;
      for (int k = 0; k < 3; k++) box.mn[k] = 3.402823466e+38f, box.mx[k] = -3.402823466e+38f;
      for (unsigned i = start; i < end; i++) {
        const float* b = lboxes + 6 * (size_t)i;
        for (int k = 0; k < 3; k++) box.mn[k] = fmin_(box.mn[k], b[k]), box.mx[k] = fmax_(box.mx[k], b[3 + k]);
      }
    } else {  // the child node's W slots, united pairwise as the L binary levels they stand for unite their children
      const float4* child = blob + 2 * (size_t)ref;
      Box6          part[L + 1];
#pragma unroll
      for (int c = 0; c < W; c++) {
        const float4 lo = child[2 * c], ch = child[2 * c + 1];
        Box6         cur;
        if (__float_as_uint(ch.z) == 0xFFFFFFFFu) {
          for (int k = 0; k < 3; k++) cur.mn[k] = inf, cur.mx[k] = -inf;
        } else {
          cur.mn[0] = lo.x, cur.mn[1] = lo.y, cur.mn[2] = lo.z, cur.mx[0] = lo.w, cur.mx[1] = ch.x, cur.mx[2] = ch.y;
        }
        int level = 0;
#pragma unroll
        for (int bit = 0; bit < L; bit++)
          if (level == bit && ((c >> bit) & 1)) cur = unite(part[bit], cur), level = bit + 1;
        part[level] = cur;
      }
      box = part[L];
    }
    node[2 * s] = make_float4(box.mn[0], box.mn[1], box.mn[2], box.mx[0]);
    *(float2*)&node[2 * s + 1] = make_float2(box.mx[1], box.mx[2]);
  }
}

// partial[block] = sum over the block's strided share of nodes of the half-areas of their occupied slot boxes, in double
__global__ void k_area_partials(int W, const float4* blob, unsigned int node_off, int count, double* partial) {
  __shared__ double sh[RB];
  double            sum = 0;
  for (size_t i = (size_t)blockIdx.x * RB + threadIdx.x; i < (size_t)count; i += (size_t)gridDim.x * RB) {
    const float4* node = blob + 2 * ((size_t)node_off + (size_t)W * i);
    for (int s = 0; s < W; s++) {
      const float4 lo = node[2 * s], hi = node[2 * s + 1];
      if (__float_as_uint(hi.z) == 0xFFFFFFFFu) continue;
      const double dx = (double)lo.w - (double)lo.x, dy = (double)hi.x - (double)lo.y, dz = (double)hi.y - (double)lo.z;
      sum += dx * dy + dy * dz + dz * dx;
    }
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (int half = RB / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) sh[threadIdx.x] += sh[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// The first wide node of every level of the three wide trees: wide level k of width 2^L holds the flagged nodes of binary level k * L, so its first
// index is the scan's value (widx: the wide index of every binary node, csrc/bvh_gpu.hip) at that level's first node. Block w = width 4 << w;
// out[66 * w + k], k = 0 .. wide_levels[w] - 1, then the count.
struct LevelFirsts {
  int                 first[3][66], wide_levels[3];
  const unsigned int* widx[3];
};
__global__ void k_wide_level_firsts(int num_nodes, LevelFirsts at, unsigned int* out) {
  const int w = blockIdx.x, k = threadIdx.x;
  if (k > at.wide_levels[w]) return;
  out[66 * w + k] = at.widx[w][k < at.wide_levels[w] ? at.first[w][k] : num_nodes];
}

unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// levels, level_first: the binary tree's (HOST); d_widx[w]: the index yhk_wide_index made for width 4 << w; d_out: 3 x 66 words of device
// memory; wide_levels[w] and wide_first[w][0 .. wide_levels[w]] on the HOST (the last one the count). One launch, one copy; synchronises.
extern "C" int yhk_wide_level_firsts(int num_nodes, int levels, const int* level_first, const unsigned int* const d_widx[3], unsigned int* d_out, int wide_levels[3],
    int wide_first[3][66], hipStream_t stream) {
  if (levels < 1 || levels > 128) return (int)hipErrorInvalidValue;
  LevelFirsts at;
  for (int w = 0; w < 3; w++) {
    const int L = 2 + w;
    at.wide_levels[w] = wide_levels[w] = 1 + std::max(0, levels - 2) / L, at.widx[w] = d_widx[w];
    for (int k = 0; k < wide_levels[w]; k++) at.first[w][k] = level_first[k * L];  // (k * L <= levels - 2: a level of the binary tree)
  }
  unsigned int host[3 * 66];
  hipLaunchKernelGGL(k_wide_level_firsts, dim3(3), dim3(128), 0, stream, num_nodes, at, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host, d_out, sizeof(host), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return (int)e;
  for (int w = 0; w < 3; w++)
    for (int k = 0; k <= wide_levels[w]; k++) wide_first[w][k] = (int)host[66 * w + k];
  return 0;
}

// how many partials the two reductions write for n items (a function of n alone: the sums are the same from run to run)
extern "C" int yhk_refit_partials(int n) { return (int)std::max(1ll, std::min(256ll, ((long long)n + RB - 1) / RB)); }

// recs: the shape's FIRST leaf record (device); boxes: n x 6 floats (device), leaf order; all arrays device arrays
extern "C" int yhk_refit_boxes(int lines, int n, const void* recs, const float* pos, const float* radius, const int* idx, float* boxes, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_refit_boxes, dim3(blocks(n)), dim3(256), 0, stream, lines, n, (const float4*)recs, pos, radius, idx, boxes);
  return (int)hipGetLastError();
}
// partial: yhk_refit_partials(n) x 6 floats (device)
extern "C" int yhk_box_partials(int n, const float* boxes, float* partial, hipStream_t stream) {
  hipLaunchKernelGGL(k_box_partials, dim3((unsigned)yhk_refit_partials(n)), dim3(RB), 0, stream, n, boxes, partial);
  return (int)hipGetLastError();
}
extern "C" int yhk_refit_records(int lines, int n, const float* pos, const float* nrm, const float* radius, const int* idx, void* recs, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_refit_records, dim3(blocks(n)), dim3(256), 0, stream, lines, n, pos, nrm, radius, idx, (float4*)recs);
  return (int)hipGetLastError();
}
// One width of one shape, every level: level_first[l] = the first wide node of wide level l, level_first[levels] = the node count
extern "C" int yhk_refit_wide(int L, void* blob, long long node_off, long long test_off, int units, int levels, const int* level_first, const float* lboxes, hipStream_t stream) {
  if (L < 2 || L > 4 || levels < 1 || units < 1) return (int)hipErrorInvalidValue;
  for (int l = levels - 1; l >= 0; l--) {
    const int first = level_first[l], count = level_first[l + 1] - first;
    if (count <= 0) continue;
    dim3 g((unsigned)((count + 127) / 128)), t(128);
    if (L == 2) hipLaunchKernelGGL(k_refit_wide<2>, g, t, 0, stream, (float4*)blob, (unsigned)node_off, first, count, (unsigned)test_off, (unsigned)units, lboxes);
    else if (L == 3) hipLaunchKernelGGL(k_refit_wide<3>, g, t, 0, stream, (float4*)blob, (unsigned)node_off, first, count, (unsigned)test_off, (unsigned)units, lboxes);
    else hipLaunchKernelGGL(k_refit_wide<4>, g, t, 0, stream, (float4*)blob, (unsigned)node_off, first, count, (unsigned)test_off, (unsigned)units, lboxes);
  }
  return (int)hipGetLastError();
}
// partial: yhk_refit_partials(count) doubles (device)
extern "C" int yhk_area_partials(int width, const void* blob, long long node_off, int count, double* partial, hipStream_t stream) {
  hipLaunchKernelGGL(k_area_partials, dim3((unsigned)yhk_refit_partials(count)), dim3(RB), 0, stream, width, (const float4*)blob, (unsigned)node_off, count, partial);
  return (int)hipGetLastError();
}
