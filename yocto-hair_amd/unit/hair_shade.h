// hair_shade.h — the body of the unit-level hair kernels (yh_hair_shade_batch): what a shaded hair hit runs in the sample loops
// (dev_path.h: path_step, shade_step), row by row, on the material row the upload makes (host/scene_upload.cpp: make_material).
//
// Compiled twice, as the sample loop is: unit/hair_shade.hip with the default arithmetic (YH_HAIR_FAST = 1, both forms),
// unit/hair_shade_exact.hip with YH_HAIR_FAST = 0 (the quad form only: the product runs the exact arithmetic as the quad kernel alone).
// Each includes this header once, after naming its kernel and launcher (YH_HAIR_SHADE_KERNEL, YH_HAIR_SHADE_LAUNCH): device functions
// are inline and per translation unit, so the two arithmetics never mix (csrc/exact.hip).
//
// The sequence per row, with QUAD = !YH_LANE of dev_path.h:
//     hh = hair_setup<QUAD>(v, normal, tangent);  ho = hair_prepare<QUAD>(mat, hh, outgoing);      dev_path.h:643-644
//     sampled = hair_sample(mat, hh, ho, rnx, rny);                                                 dev_path.h:653
//     hair_eval_pdf_quad / hair_eval_pdf_lane(mat, hh, ho, incoming, f, pdf)                        dev_path.h:672-676
// the last once at `incoming` and once at the sampled direction.
// out, YH_HAIR_SHADE_FLOATS per row: f[3] pdf at `incoming`, sampled[3], f[3] pdf at the sampled direction, ho.pdf0..3.
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "dev_hair.h"

using namespace yhd;

template <bool QUAD>
YH_DEV void hair_shade_row(const yhd_material& mat, float v, f3 normal, f3 tangent, f3 outgoing, f3 incoming, float rnx, float rny,
    bool write, float* o) {
  hair_hit hh      = hair_setup<QUAD>(v, normal, tangent);
  hair_out ho      = hair_prepare<QUAD>(mat, hh, outgoing);
  f3       sampled = hair_sample(mat, hh, ho, rnx, rny);
  f3       f, fs;
  float    pdf, pdfs;
  if constexpr (QUAD) {
    hair_eval_pdf_quad(mat, hh, ho, incoming, f, pdf);
    hair_eval_pdf_quad(mat, hh, ho, sampled, fs, pdfs);
  } else {
    hair_eval_pdf_lane(mat, hh, ho, incoming, f, pdf);
    hair_eval_pdf_lane(mat, hh, ho, sampled, fs, pdfs);
  }
  if (!write) return;
  o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = pdf;
  o[4] = sampled.x, o[5] = sampled.y, o[6] = sampled.z;
  o[7] = fs.x, o[8] = fs.y, o[9] = fs.z, o[10] = pdfs;
  o[11] = ho.pdf0, o[12] = ho.pdf1, o[13] = ho.pdf2, o[14] = ho.pdf3;
}

// QUAD: four threads per row, 64 rows per block; else a thread per row
template <bool QUAD>
__global__ __launch_bounds__(256) void YH_HAIR_SHADE_KERNEL(int n, const yhd_material* mats, const float* v, const float* normal,
    const float* tangent, const float* outgoing, const float* incoming, const float* rn, float* out) {
  int  i     = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> (QUAD ? 2 : 0);
  bool valid = i < n;
  if (!valid) {
    if (!QUAD) return;
    i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  }
  const size_t r = (size_t)i;
  hair_shade_row<QUAD>(mats[r], v[r], ld3(normal + 3 * r), ld3(tangent + 3 * r), ld3(outgoing + 3 * r), ld3(incoming + 3 * r),
      rn[2 * r], rn[2 * r + 1], valid && (!QUAD || (threadIdx.x & 3) == 0), out + YH_HAIR_SHADE_FLOATS * r);
}

extern "C" int YH_HAIR_SHADE_LAUNCH(int form, int n, const void* mats, const float* v, const float* normal, const float* tangent,
    const float* outgoing, const float* incoming, const float* rn, float* out, hipStream_t s) {
  if (n < 1 || (form != 0 && !(YH_HAIR_FAST && form == 1))) return (int)hipErrorInvalidValue;
  if (form == 0) {
    hipLaunchKernelGGL(YH_HAIR_SHADE_KERNEL<true>, dim3((n + 63) / 64), dim3(256), 0, s, n, (const yhd_material*)mats, v, normal,
        tangent, outgoing, incoming, rn, out);
  } else {
#if YH_HAIR_FAST
    hipLaunchKernelGGL(YH_HAIR_SHADE_KERNEL<false>, dim3((n + 255) / 256), dim3(256), 0, s, n, (const yhd_material*)mats, v, normal,
        tangent, outgoing, incoming, rn, out);
#endif
  }
  return (int)hipGetLastError();
}
