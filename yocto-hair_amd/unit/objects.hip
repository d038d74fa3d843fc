// objects.hip — yh_update_objects: what a moved object changes in its row of the object table, on the device, one lane per edited row:
// the frame, its inverse (inverse(frame, non_rigid = true), pt.cpp:1012-1013), the material, and the object's world box —
// transform_bbox of its shape's root box (pt.cpp:806) — once as it is (the host builds the scene-level tree over those) and once with the
// upload's margin (yhd_object::wbox_min / wbox_max). The arithmetic is unit/object_math.h, the text the upload runs on the host, and
// both builds keep a multiply and an add apart, so a row written here holds the bits an upload of the edited description puts there.
// A translation unit of its own: the sample-loop units do not see it. Not a hot path in the kernels' sense: IEEE division, no LDS.
#include <hip/hip_runtime.h>

#include "../csrc/yh_device.h"
#include "../csrc/launchers.h"
#include "object_math.h"
#include "yhair.h"

namespace {

static_assert(sizeof(yh_object) == 56, "rows are passed as the C ABI's yh_object");

__global__ void k_object_rows(int count, const yh_object* rows, const float* root6, yhd_object* objects, float* boxes6) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count) return;
  const yh_object row = rows[i];
  const float*    b   = root6 + 6 * (size_t)row.shape;  // (the host checked the shape: it is the uploaded row's)
  float bmin[3] = {b[0], b[1], b[2]}, bmax[3] = {b[3], b[4], b[5]};
  float lo[3], hi[3];
  transform_bbox(row.frame, bmin, bmax, lo, hi);
  for (int k = 0; k < 3; k++) boxes6[6 * (size_t)i + k] = lo[k], boxes6[6 * (size_t)i + 3 + k] = hi[k];
  if (!objects) return;
  yhd_object& d = objects[i];
  float inv[12], wmin[4], wmax[4];
  inverse_frame(row.frame, true, inv);
  padded_world_box(lo, hi, wmin, wmax);
  for (int k = 0; k < 12; k++) d.frame[k] = row.frame[k], d.inv_frame[k] = inv[k];
  for (int k = 0; k < 4; k++) d.wbox_min[k] = wmin[k], d.wbox_max[k] = wmax[k];
  d.material = row.material;
}

}  // namespace

// rows: `count` yh_object in device memory; root6: 6 floats per shape; objects: the first of the `count` rows of the object table to
// rewrite, or NULL (boxes only); boxes6: 6 floats per row
extern "C" int yhk_object_rows(int count, const void* rows, const float* root6, void* objects, float* boxes6, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(k_object_rows, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, count, (const yh_object*)rows, root6, (yhd_object*)objects, boxes6);
  return (int)hipGetLastError();
}
