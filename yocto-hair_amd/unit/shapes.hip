// shapes.hip — yh_update_shape / yh_update_shape_device: the per-element work of a vertex edit beyond the builder's (csrc/bvh_gpu.hip), on
// the device, one lane per element:
//   k_index_check        whether an index of the shape lies outside [0, num_vertices): one flag word, set through a (vector) atomic. It
//                        runs before anything reads a vertex through an index — the device form's arrays never visit the host, and
//                        the host form uses it too, so that both refuse alike;
//   k_vertex_rows,       the shape's rows of the per-vertex arrays a launch reads to sample a point on a triangle and to interpolate
//   k_element_rows       texture coordinates (yhd_scene::vpos, vtex, elems): copies and the default radius only, the upload's bits
//                        (host/scene_upload.cpp: the per-vertex section);
//   k_object_lane_roots  where the shape's 4- / 8- / 16-wide nodes begin, in the rows of the objects that name it. CHOSEN over a wider
//                        yhk_object_rows: that kernel stays the one yh_update_objects was tested with, and the roots are three stores.
// A translation unit of its own: the sample-loop units do not see it. Not a hot path in the kernels' sense: no LDS, plain C++.
#include <hip/hip_runtime.h>

#include "../csrc/yh_device.h"
#include "../csrc/launchers.h"
#include "yhair.h"

namespace {

static_assert(sizeof(yh_object) == 56, "rows are passed as the C ABI's yh_object");

__global__ void k_index_check(int n, const int* idx, int num_vertices, unsigned int* flag) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)n) return;
  const int v = idx[k];
  if (v < 0 || v >= num_vertices) atomicOr(flag, 1u);
}

__global__ void k_vertex_rows(int lines, int num_vertices, const float* pos, const float* radius, const float* texcoords, float4* vpos, float2* vtex) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= (size_t)num_vertices) return;
  const float w = lines ? (radius ? radius[v] : 0.001f) : 0.0f;  // add_radius, sceneio.cpp:390
  vpos[v] = make_float4(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2], w);
  vtex[v] = texcoords ? make_float2(texcoords[2 * v], texcoords[2 * v + 1]) : make_float2(0.0f, 0.0f);
}

__global__ void k_element_rows(int lines, int num_elems, const int* idx, int4* elems) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)num_elems) return;
  elems[e] = lines ? make_int4(idx[2 * e], idx[2 * e + 1], 0, 0) : make_int4(idx[3 * e], idx[3 * e + 1], idx[3 * e + 2], 0);
}

__global__ void k_object_lane_roots(int count, const yh_object* rows, int shape, int root4, int root8, int root16, yhd_object* objects) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count || rows[i].shape != shape) return;
  objects[i].lane_root = root4, objects[i].lane_root8 = root8, objects[i].lane_root16 = root16;
}

unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// idx: n indices; flag: one word of device memory, cleared here; *bad on the host: 1 when an index lies outside [0, num_vertices)
extern "C" int yhk_index_check(int n, const int* idx, int num_vertices, unsigned int* flag, int* bad, hipStream_t stream) {
  *bad = 0;
  if (n <= 0) return 0;
  hipError_t e = hipMemsetAsync(flag, 0, 4, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_index_check, dim3(blocks(n)), dim3(256), 0, stream, n, idx, num_vertices, flag);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  unsigned int word = 0;
  if ((e = hipMemcpyAsync(&word, flag, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return (int)e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return (int)e;
  *bad = word != 0;
  return 0;
}

// vpos (float4), vtex (2 floats) and elems (int4): the FIRST row of the shape in each array; radius and texcoords may be NULL
extern "C" int yhk_vertex_rows(int lines, int num_vertices, int num_elems, const float* pos, const float* radius, const float* texcoords, const int* idx,
    void* vpos, float* vtex, void* elems, hipStream_t stream) {
  if (num_vertices > 0)
    hipLaunchKernelGGL(k_vertex_rows, dim3(blocks(num_vertices)), dim3(256), 0, stream, lines, num_vertices, pos, radius, texcoords, (float4*)vpos, (float2*)vtex);
  if (num_elems > 0) hipLaunchKernelGGL(k_element_rows, dim3(blocks(num_elems)), dim3(256), 0, stream, lines, num_elems, idx, (int4*)elems);
  return (int)hipGetLastError();
}

// rows: `count` yh_object in device memory (the whole object list); objects: the object table's first row
extern "C" int yhk_object_lane_roots(int count, const void* rows, int shape, int root4, int root8, int root16, void* objects, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(k_object_lane_roots, dim3(blocks(count)), dim3(256), 0, stream, count, (const yh_object*)rows, shape, root4, root8, root16, (yhd_object*)objects);
  return (int)hipGetLastError();
}
