// framebuffer.hip — the accumulated image out of the render state (gfx950): resolved into a full W x H image (every download), and the
// tile-packed float4 framebuffer of the gather (yh_gather_framebuffer). One wave per 8 x 8 tile. Outside csrc/, as every kernel that is
// not a sample loop. Compiled with -ffp-contract=off: the divisions are IEEE.
#include <hip/hip_runtime.h>

#include "launchers.h"

// render[ij] = accumulated / samples (pt.cpp:1688) into a full W*H image
__global__ void k_resolve(const yhd_state st, int samples, yhd_float4* image) {
  // block k handles the k-th tile owned by this shard: tile id rank + k * world
  int lane = threadIdx.x;
  int tile = st.shard_rank + blockIdx.x * st.shard_world;
  int i    = (tile % st.tiles_x) * YH_TILE + (lane & 7);
  int j    = (tile / st.tiles_x) * YH_TILE + (lane >> 3);
  if (i >= st.width || j >= st.height) return;
  size_t     pix = (size_t)j * st.width + i;
  yhd_float4 a   = st.accum[pix];
  float      n   = (float)samples;
  image[pix]     = samples > 0 ? yhd_float4{a.x / n, a.y / n, a.z / n, a.w / n} : yhd_float4{0, 0, 0, 0};
}
// tile-packed variant: 64 float4 per owned tile, tiles in increasing id order
__global__ void k_pack(const yhd_state st, int samples, yhd_float4* packed) {
  int lane = threadIdx.x;
  int tile = st.shard_rank + blockIdx.x * st.shard_world;
  int i    = (tile % st.tiles_x) * YH_TILE + (lane & 7);
  int j    = (tile / st.tiles_x) * YH_TILE + (lane >> 3);
  yhd_float4 out = {0, 0, 0, 0};
  if (i < st.width && j < st.height && samples > 0) {
    yhd_float4 a = st.accum[(size_t)j * st.width + i];
    float      n = (float)samples;
    out          = yhd_float4{a.x / n, a.y / n, a.z / n, a.w / n};
  }
  packed[(size_t)blockIdx.x * 64 + lane] = out;
}
__global__ void k_unpack(const yhd_float4* packed, int src_rank, int world, int num_tiles_total,
    int tiles_x, int width, int height, yhd_float4* image) {
  // the k-th tile owned by src_rank is tile id src_rank + k * world
  int k = blockIdx.x, lane = threadIdx.x;
  int tile = src_rank + k * world;
  if (tile >= num_tiles_total) return;
  int i = (tile % tiles_x) * YH_TILE + (lane & 7);
  int j = (tile / tiles_x) * YH_TILE + (lane >> 3);
  if (i < width && j < height) image[(size_t)j * width + i] = packed[(size_t)k * 64 + lane];
}

extern "C" {
int yhk_resolve(const yhd_state* st, int owned_tiles, int samples, void* image, hipStream_t stream) {
  if (owned_tiles) hipLaunchKernelGGL(k_resolve, dim3(owned_tiles), dim3(64), 0, stream, *st, samples, (yhd_float4*)image);
  return (int)hipGetLastError();
}
int yhk_pack(const yhd_state* st, int owned_tiles, int samples, void* packed, hipStream_t stream) {
  if (owned_tiles) hipLaunchKernelGGL(k_pack, dim3(owned_tiles), dim3(64), 0, stream, *st, samples, (yhd_float4*)packed);
  return (int)hipGetLastError();
}
int yhk_unpack(const void* packed, int src_rank, int world, int ntiles_src, int num_tiles_total, int tiles_x,
    int width, int height, void* image, hipStream_t stream) {
  if (ntiles_src)
    hipLaunchKernelGGL(k_unpack, dim3(ntiles_src), dim3(64), 0, stream, (const yhd_float4*)packed, src_rank, world,
        num_tiles_total, tiles_x, width, height, (yhd_float4*)image);
  return (int)hipGetLastError();
}
}
