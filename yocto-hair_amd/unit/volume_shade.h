// volume_shade.h — the body of the unit-level volume kernels (yh_volume_batch): what a path runs in a homogeneous medium in the sample
// loops (dev_path.h: medium_crossing and the free-flight block of path_step), row by row, on the material row the upload makes
// (host/scene_upload.cpp: make_material). Every step calls the device functions of dev_path.h / dev_surface.h themselves.
//
// Compiled twice, as the sample loop is: unit/volume_quad.hip (a quad per row, as k_trace<GENERAL> runs it) and unit/volume_lane.hip
// with YH_LANE 1 (a lane per row, as k_stream runs it: the medium goes through the path's slot, medium_mem, and is read back from it
// as the free-flight block of path_step reads it).
//
// The sequence per row:
//     medium_crossing(sc, ps, mat, normal, outgoing, incoming, color_tex, emission_tex_x, 0, 0)     from outside, ps.medium zeroed
//     dist = sample_transmittance(ps.medium.density, max_distance, rl, rd)                          dev_path.h: path_step, free flight
//     eval_transmittance(density, dist) / sample_transmittance_pdf(density, dist, max_distance)
//     sampled = sample_scattering(ps.medium, outgoing, rx, ry)                                      ... scatter
//     eval_scattering, sample_scattering_pdf at `incoming` and at `sampled`
// A row whose crossing enters no medium (thin, no transmission, both directions on one side) runs the rest on the zeroed medium.
// out, YH_VOLUME_FLOATS per row: in_medium, density[3], scatter[3], anisotropy, distance, weight factor[3], distance pdf,
// sampled[3], f[3] pdf at `incoming`, f[3] pdf at the sampled direction.
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "dev_path.h"

using namespace yhd;

YH_DEV void volume_row(const yhd_scene& sc, const yhd_material& mat, f3 normal, f3 outgoing, f3 incoming, f3 color_tex, float emission_tex_x,
    float rl, float rd, float max_distance, float rx, float ry, yhd_float4* slot, bool write, float* o) {
  path_t ps;
  ps.in_medium      = false;
  ps.medium.density = mk3(0.0f), ps.medium.scatter = mk3(0.0f), ps.medium.anisotropy = 0.0f;
#if YH_LANE
  ps.medium_mem = slot;
#endif
  medium_crossing(sc, ps, mat, normal, outgoing, incoming, color_tex, emission_tex_x, 0.0f, 0.0f);
#if YH_LANE
  if (ps.in_medium) {  // (as path_step: the medium comes back from the path's slot)
    const yhd_float4 m0 = ps.medium_mem[0], m1 = ps.medium_mem[1];
    ps.medium.density = f3{m0.x, m0.y, m0.z}, ps.medium.anisotropy = m0.w, ps.medium.scatter = f3{m1.x, m1.y, m1.z};
  }
#endif
  const float dist    = sample_transmittance(ps.medium.density, max_distance, rl, rd);
  const float tpdf    = sample_transmittance_pdf(ps.medium.density, dist, max_distance);
  const f3    w       = eval_transmittance(ps.medium.density, dist) / tpdf;
  const f3    sampled = sample_scattering(ps.medium, outgoing, rx, ry);
  const f3    f       = eval_scattering(ps.medium, outgoing, incoming);
  const float pdf     = sample_scattering_pdf(ps.medium, outgoing, incoming);
  const f3    fs      = eval_scattering(ps.medium, outgoing, sampled);
  const float pdfs    = sample_scattering_pdf(ps.medium, outgoing, sampled);
  if (!write) return;
  o[0] = ps.in_medium ? 1.0f : 0.0f;
  o[1] = ps.medium.density.x, o[2] = ps.medium.density.y, o[3] = ps.medium.density.z;
  o[4] = ps.medium.scatter.x, o[5] = ps.medium.scatter.y, o[6] = ps.medium.scatter.z, o[7] = ps.medium.anisotropy;
  o[8] = dist, o[9] = w.x, o[10] = w.y, o[11] = w.z, o[12] = tpdf;
  o[13] = sampled.x, o[14] = sampled.y, o[15] = sampled.z;
  o[16] = f.x, o[17] = f.y, o[18] = f.z, o[19] = pdf;
  o[20] = fs.x, o[21] = fs.y, o[22] = fs.z, o[23] = pdfs;
}

// texval: 4 per row (the colour texture's value[3], the emission texture's x); rn: 5 per row (rl, rd, max_distance, rx, ry);
// slots: two float4 per row (the lane form's medium_mem)
__global__ __launch_bounds__(256) void YH_VOLUME_KERNEL(const yhd_scene sc, int n, const yhd_material* mats, const float* normal,
    const float* outgoing, const float* incoming, const float* texval, const float* rn, yhd_float4* slots, float* out) {
  constexpr bool QUAD = !YH_LANE;
  int  i     = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> (QUAD ? 2 : 0);
  bool valid = i < n;
  if (!valid) {
    if (!QUAD) return;
    i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  }
  const size_t r = (size_t)i;
  const float* t = texval + 4 * r;
  const float* q = rn + 5 * r;
  volume_row(sc, mats[r], ld3(normal + 3 * r), ld3(outgoing + 3 * r), ld3(incoming + 3 * r), ld3(t), t[3], q[0], q[1], q[2], q[3], q[4],
      slots + 2 * r, valid && (!QUAD || (threadIdx.x & 3) == 0), out + YH_VOLUME_FLOATS * r);
}

// sc: no texture is looked up (the rows' scattering_tex is -1), so an empty scene serves
extern "C" int YH_VOLUME_LAUNCH(const yhd_scene* sc, int n, const void* mats, const float* normal, const float* outgoing,
    const float* incoming, const float* texval, const float* rn, void* slots, float* out, hipStream_t s) {
  if (n < 1) return (int)hipErrorInvalidValue;
  const int rows_per_block = YH_LANE ? 256 : 64;
  hipLaunchKernelGGL(YH_VOLUME_KERNEL, dim3((n + rows_per_block - 1) / rows_per_block), dim3(256), 0, s, *sc, n, (const yhd_material*)mats,
      normal, outgoing, incoming, texval, rn, (yhd_float4*)slots, out);
  return (int)hipGetLastError();
}
