// volume_quad.hip — the homogeneous-medium code with a quad per row (gfx950): form 0 of yh_volume_batch, what k_trace<GENERAL> runs; and the
// quad forms of the trimmed 512-thread kernels next to the plain forms they stand for (yh_quad_forms_batch). A translation unit of its
// own, outside csrc/, as unit/lights_quad.hip.
#define YH_VOLUME_KERNEL k_volume_quads
#define YH_VOLUME_LAUNCH yhk_volume_quads
#include "launchers.h"
#include "volume_shade.h"

// sample_hemisphere_cos_quad (dev_surface.h) next to sample_hemisphere_cos, quad_div (dev_math.h) next to a / b: a quad per row, all
// four lanes active on identical operands, as the trimmed shading pass calls them (dev_path.h: path_step<TRIM>).
// out, YH_QUAD_FORMS_FLOATS per row: sample_hemisphere_cos_quad[3], sample_hemisphere_cos[3], quad_div(a, b)[3], a / b [3].
__global__ __launch_bounds__(256) void k_quad_forms(int n, const float* normal, const float* rn, const float* a, const float* b, float* out) {
  int  i     = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  bool valid = i < n;
  if (!valid) i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  const size_t r  = (size_t)i;
  const f3     nn = ld3(normal + 3 * r), av = ld3(a + 3 * r);
  const float  rx = rn[2 * r], ry = rn[2 * r + 1], bv = b[r];
  const f3     hq = sample_hemisphere_cos_quad(nn, rx, ry);
  const f3     hp = sample_hemisphere_cos(nn, rx, ry);
  const f3     dq = quad_div(av, bv);
  const f3     dp = av / bv;
  if (valid && (threadIdx.x & 3) == 0) {
    float* o = out + YH_QUAD_FORMS_FLOATS * r;
    o[0] = hq.x, o[1] = hq.y, o[2] = hq.z, o[3] = hp.x, o[4] = hp.y, o[5] = hp.z;
    o[6] = dq.x, o[7] = dq.y, o[8] = dq.z, o[9] = dp.x, o[10] = dp.y, o[11] = dp.z;
  }
}

extern "C" int yhk_quad_forms(int n, const float* normal, const float* rn, const float* a, const float* b, float* out, hipStream_t s) {
  if (n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_quad_forms, dim3((n + 63) / 64), dim3(256), 0, s, n, normal, rn, a, b, out);
  return (int)hipGetLastError();
}
