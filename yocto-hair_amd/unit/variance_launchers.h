// variance_launchers.h — the yhk_* functions of unit/variance.hip, declared ONCE for both compilers as csrc/launchers.h declares every
// other unit's: the host includes this header (host/image_pass.h) and so does unit/variance.hip, so a declaration that disagreed with its
// definition does not build. They are here and not in csrc/launchers.h because the headers of csrc/ are part of the device code's
// fingerprint (bench.py: csrc_sha16, the key of the committed counter passes in profiles/k_trace_traffic.json): a unit outside csrc/
// that adds kernels of its own leaves that text, and with it the passes' claim to describe the kernels in the tree, as it was.
#ifndef YH_VARIANCE_LAUNCHERS_H_
#define YH_VARIANCE_LAUNCHERS_H_
#include "../csrc/launchers.h"

extern "C" {
// unit/variance.hip (yh_temporal_accumulate_variance ..., include/yhair.h: VARIANCE), pointers as yhk_reproject and yhk_dn_level take them.
// Stage M: yhk_reproject's step with the moment history hm = {M1, M2, steps bits, vt} carried beside hc / hg (albedo NULL: none; hm_in
// NULL: no moment history; hm_out is not hm_in). Stage S: the variance of every pixel from a step's hm / hg. yhk_var_steps: the steps of
// a moment plane as ints. Stage F: the pack step with the variance in u.w, and one level in form 0 or 1 as yhk_dn_level has them; the
// last level takes the alpha of alpha_src (a float4 image) / alpha_div and writes the variance plane (NULL: not).
int yhk_reproject_m(const void* rgba_in, const void* accum, int samples, const int* object, const float* position, const float* albedo, int width, int height,
    const void* hc_in, const void* hg_in, const void* hm_in, int have_history, const float* cam, const float* pcam, const void* motion,
    const yh_temporal_params* P, void* hc_out, void* hg_out, void* hm_out, void* rgba_out, hipStream_t);
int yhk_var_spatial(int width, int height, const yh_temporal_params* T, int min_steps, const void* hm, const void* hg, float* variance, hipStream_t);
int yhk_var_steps(const void* hm, int width, int height, int* steps, hipStream_t);
int yhk_vdn_pack(const void* rgba_in, const void* accum, int samples, int width, int height, const float* variance, const int* object, const float* normal,
    const float* position, const float* albedo, void* u, void* g0, void* g1, hipStream_t);
int yhk_vdn_level(int form, int width, int height, int level, const yh_variance_params* P, const void* u, const void* g0, const void* g1, const float* albedo,
    int last, const void* alpha_src, float alpha_div, void* out, float* out_variance, hipStream_t);
}
#endif
