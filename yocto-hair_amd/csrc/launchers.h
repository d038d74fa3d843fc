// launchers.h — every yhk_* function the hipcc-compiled files define for the g++-compiled host code, declared ONCE: the host includes
// this header (host/context_internal.h) and so does every .hip file that defines one of them. The functions have C linkage, so a
// declaration that disagreed with its definition would still link and pass garbage; with both sides compiling these lines, two
// declarations of one name with different parameters are a compile error. Grouped by the file that defines them.
#ifndef YH_LAUNCHERS_H_
#define YH_LAUNCHERS_H_
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "yh_device.h"
#include "yhair.h"

// a sample-loop kernel (csrc/dev_items.h: k_trace and its kin)
typedef void (*trace_kernel_t)(const yhd_scene, const yhd_state, int, yhd_counters*);

extern "C" {
// csrc/kernels.hip: the quad sample loops. `shape`: a k_trace one (quad or wide); the caller built the work list for it
int yhk_trace(const yhd_scene*, const yhd_state*, int nsamples, yhd_counters*, int shape, int grid_blocks, hipStream_t);
int yhk_block_threads(int shape);
int yhk_stack_entries(void);
int yhk_trace_lds_bytes(const yhd_scene* sc, int shape);
int yhk_trace_occupancy(int lds_bytes, int general, int shape);
// csrc/wide.hip: the wide launch shapes (their kernel for yhk_trace, or NULL when this build does not contain it) and the side-by-side launch
trace_kernel_t yhk_wide_kernel(int counted, int general, int shape);
int yhk_trace_sbs(const yhd_scene*, const yhd_state*, int nsamples, int oct_blocks, int quad_items, int oct_entries, int grid_blocks, hipStream_t);
int yhk_trace_sbs_lds_bytes(const yhd_scene* sc);
int yhk_trace_sbs_occupancy(int lds_bytes, int general);
// csrc/exact.hip
int yhk_trace_exact(const yhd_scene*, const yhd_state*, int nsamples, int lds_bytes, int grid_blocks, hipStream_t);
int yhk_trace_exact_occupancy(int lds_bytes, int general);
// csrc/stream.hip
int yhk_stream(const yhd_scene*, const yhd_scene* sc_dev, const yhd_state*, int nsamples, const yhd_stream*, int grid_blocks, hipStream_t);
int yhk_lane_tests(const yhd_float4* prims, yhd_float4* blob, int kind, int prim_base, int num_prims, long long test_off, hipStream_t);
int yhk_stream_block_threads(void);
int yhk_stream_lds_bytes(int tables_f4, int slots_per_wave);
int yhk_stream_occupancy(int lds_bytes, int general);
int yhk_intersect_lanes_lds(const yhd_scene* sc);
int yhk_intersect_lanes_occupancy(const yhd_scene* sc, int waves);
int yhk_intersect_lanes(const yhd_scene* sc, const yhd_scene* sc_dev, int n, const float* rays, int* cursor, unsigned int* stack_ovf,
    int ovf_entries, int* object, int* element, float* uv, float* dist, int waves, int grid_blocks, hipStream_t stream);
// csrc/bvh_gpu.hip
int yhk_bvh_build_gpu(int n, const float* boxes, float* nodes8, int* primitives, int* num_nodes, int* depth, hipStream_t);
// ... device in / device out (yh_upload_scene): bounds, the tree, the leaf records and the wide collapses of one shape
int yhk_prim_boxes(int lines, int n, const float* pos, const float* radius, const int* idx, float* boxes, hipStream_t);
int yhk_bvh_build_resident(int n, const float* d_boxes, float* d_nodes, int* d_pid, int* num_nodes, int* levels, int* level_first, hipStream_t);
int yhk_leaf_records(int lines, int n, const int* pid, const float* pos, const float* nrm, const float* radius, const int* idx, void* prims_out, hipStream_t);
int yhk_wide_index(int num_nodes, const float* d_nodes, int levels, const int* level_first, int L, unsigned int* d_flag, unsigned int* d_widx, int* count, hipStream_t);
int yhk_wide_collapse(int L, int num_nodes, const float* d_nodes, const unsigned int* d_flag, const unsigned int* d_widx, int lines, long long node_off, long long test_off, void* blob, hipStream_t);

// unit/framebuffer.hip: the accumulated image divided by its samples into a W x H image, or tile-packed for the gather, and unpacked again
int yhk_resolve(const yhd_state*, int owned_tiles, int samples, void* image, hipStream_t);
int yhk_pack(const yhd_state*, int owned_tiles, int samples, void* packed, hipStream_t);
int yhk_unpack(const void* packed, int src_rank, int world, int ntiles_src, int num_tiles_total, int tiles_x, int width, int height, void* image, hipStream_t);
// unit/hair_batch.hip (yh_hair_*_batch): mats = n rows of the public yh_material, brdf = 30 floats per item
int yhk_hair_brdf(int n, const void* mats, const float* v, const float* nrm, const float* tng, float* out, hipStream_t);
int yhk_hair_eval(int n, const float* brdf, const float* wo, const float* wi, float* out, hipStream_t);
int yhk_hair_pdf(int n, const float* brdf, const float* wo, const float* wi, float* out, hipStream_t);
int yhk_hair_sample(int n, const float* brdf, const float* wo, const float* rn, float* out, hipStream_t);
// unit/selftest.hip
int yhk_selftest(int which, float beta_m, float beta_n, uint64_t state, uint64_t inc, int count, const float* wo, double* sums, unsigned int* worst_bits, hipStream_t);
// unit/surface_batch.hip: mats = n rows of yhd_material
int yhk_surface_lobe(int kind, int n, const float* params, const float* normal, const float* wo, const float* wi, const float* rn, float* out, hipStream_t);
int yhk_surface_bsdf(int n, const void* mats, const float* normal, const float* wo, const float* wi, const float* rn, float* out, hipStream_t);
// unit/curves.hip
int yhk_curves_to_lines(int n, const float* P, const float* w0, const float* w1, int base_vertex, float* positions, float* normals, float* radius, int* lines, hipStream_t);
// unit/intersect_quad.hip, unit/intersect_wide.hip
int yhk_intersect(const yhd_scene*, int n, const float* rays, int* object, int* element, float* uv, float* dist, hipStream_t);
int yhk_intersect_plain(const yhd_scene*, int form, int n, const float* rays, int* object, int* element, float* uv, float* dist, hipStream_t);
int yhk_intersect_wide(const yhd_scene*, int form, int in_memory, int n, const float* rays, int* object, int* element, float* uv, float* dist, hipStream_t);
// unit/lights_quad.hip, unit/lights_lane.hip
int yhk_lights_lds_bytes(const yhd_scene* sc);
int yhk_lights(const yhd_scene*, int n, const float* position, const float* direction, const float* rn, float* out, hipStream_t);
int yhk_lights_lanes(const yhd_scene* sc, const yhd_scene* sc_dev, int n, const float* position, const float* direction, const float* rn,
    unsigned int* stack_ovf, int ovf_entries, float* out, hipStream_t stream);
// unit/hair_shade.hip, unit/hair_shade_exact.hip (yh_hair_shade_batch): mats = n rows of yhd_material; form 0 a quad per row, 1 a lane per row (fast only)
int yhk_hair_shade(int form, int n, const void* mats, const float* v, const float* normal, const float* tangent, const float* outgoing, const float* incoming,
    const float* rn, float* out, hipStream_t);
int yhk_hair_shade_exact(int form, int n, const void* mats, const float* v, const float* normal, const float* tangent, const float* outgoing,
    const float* incoming, const float* rn, float* out, hipStream_t);
// unit/point_quad.hip, unit/point_lane.hip (yh_point_batch): slot_of = the leaf slots by element of the shapes the batch names (yhk_point_slots: one shape,
// through an object that has it), slot_base = per object where its shape's begin there; slots = 2n float4 (the lane form's medium_mem)
int yhk_point_slots(const yhd_scene* sc, int object, int num, int* slot_of, hipStream_t);
int yhk_point_quads(const yhd_scene* sc, int form, int n, const int* object, const int* element, const int* slot_of, const int* slot_base, const float* uv,
    const float* outgoing, void* slots, float* out, hipStream_t);
int yhk_point_lanes(const yhd_scene* sc, int form, int n, const int* object, const int* element, const int* slot_of, const int* slot_base, const float* uv,
    const float* outgoing, void* slots, float* out, hipStream_t);
// unit/volume_quad.hip, unit/volume_lane.hip (yh_volume_batch): mats = n rows of yhd_material, texval 4n, rn 5n, slots = 2n float4 (the lane form's medium_mem)
int yhk_volume_quads(const yhd_scene* sc, int n, const void* mats, const float* normal, const float* outgoing, const float* incoming, const float* texval,
    const float* rn, void* slots, float* out, hipStream_t);
int yhk_volume_lanes(const yhd_scene* sc, int n, const void* mats, const float* normal, const float* outgoing, const float* incoming, const float* texval,
    const float* rn, void* slots, float* out, hipStream_t);
int yhk_quad_forms(int n, const float* normal, const float* rn, const float* a, const float* b, float* out, hipStream_t);  // unit/volume_quad.hip
// unit/path_ends_quad.hip, unit/path_ends_lane.hip (yh_path_ends_batch): op = YH_PATH_*, the rows of include/yhair.h; rng 2n (state, inc), state n
int yhk_path_ends_quads(int op, int n, const float* fin, const int* iin, const uint64_t* rng, float* fout, int* iout, uint64_t* state, hipStream_t);
int yhk_path_ends_lanes(int op, int n, const float* fin, const int* iin, const uint64_t* rng, float* fout, int* iout, uint64_t* state, hipStream_t);
// unit/display.hip
int yhk_display(const yhd_state*, int samples, float exposure, int filmic, int srgb, void* rgba8, hipStream_t);
int yhk_display_image(const void* rgba, int width, int height, float exposure, int filmic, int srgb, void* rgba8, hipStream_t);  // ... of a float4 image in device memory
// unit/gbuffer.hip (yh_trace_gbuffer): resident 256-thread workgroups per CU with the scene's LDS layout (0: the kernel cannot run); planes:
// the eleven pointers of yh_gbuffer in its order, device memory; cursor: one zeroed int; stack_ovf: ovf_entries x 64 entries for each of the
// grid's grid_blocks x 4 waves
int yhk_gbuffer_waves(void);
int yhk_gbuffer_occupancy(const yhd_scene* sc);
int yhk_gbuffer(const yhd_scene* sc, const yhd_scene* sc_dev, const yhd_state* st, int mode, void* const planes[11], int* cursor,
    unsigned int* stack_ovf, int ovf_entries, int grid_blocks, hipStream_t stream);
// unit/denoise.hip (yh_denoise ...), all pointers DEVICE pointers, float4 images 16-byte aligned: the pack step (rgba_in NULL: accum / samples;
// plain: the colour alone into u), one level of the filter in form 0 (taps from memory) or 1 (levels below yhk_dn_tiled_levels from LDS)
int yhk_dn_tile(void);
int yhk_dn_tiled_levels(void);
int yhk_dn_pack(const void* rgba_in, const void* accum, int samples, int width, int height, const int* object, const float* normal, const float* position,
    const float* albedo, void* u, void* g0, void* g1, int plain, hipStream_t);
int yhk_dn_level(int form, int width, int height, int level, const yh_denoise_params* P, const void* u, const void* g0, const void* g1, const float* albedo,
    int last, void* out, hipStream_t);
// unit/reproject.hip (yh_temporal_accumulate ...), all pointers DEVICE pointers unless said otherwise, float4 images 16-byte aligned: one step of
// the temporal stage (rgba_in NULL: accum / samples; have_history 0: the history planes are not read; cam / pcam: 17 floats on the HOST;
// motion: a yht::Motion of device pointers on the HOST, NULL: none; hc_out / hg_out are not hc_in / hg_in; rgba_out may be NULL), and
// the lengths of a history plane as ints
int yhk_reproject(const void* rgba_in, const void* accum, int samples, const int* object, const float* position, int width, int height, const void* hc_in,
    const void* hg_in, int have_history, const float* cam, const float* pcam, const void* motion, const yh_temporal_params* P, void* hc_out, void* hg_out,
    void* rgba_out, hipStream_t);
int yhk_tp_lengths(const void* hc, int width, int height, int* lengths, hipStream_t);
// unit/objects.hip (yh_update_objects): a lane per row of `rows` (yh_object, device memory); root6 = per shape its root box, 6 floats; writes
// frame, inv_frame, material and the padded world box into objects[0 .. count) unless NULL, and the world box proper, 6 floats per row, to boxes6
int yhk_object_rows(int count, const void* rows, const float* root6, void* objects, float* boxes6, hipStream_t);
// unit/shapes.hip (yh_update_shape), all pointers DEVICE pointers: whether one of n indices lies outside [0, num_vertices) (*bad on the
// host; synchronises); a shape's rows of the per-vertex arrays — vpos {p.xyz, radius or 0.001 for lines, 0 for triangles}, vtex (zeros
// without texcoords), elems — written at the shape's bases; and the three lane roots in the rows of the objects that name `shape`
int yhk_index_check(int n, const int* idx, int num_vertices, unsigned int* flag, int* bad, hipStream_t);
int yhk_vertex_rows(int lines, int num_vertices, int num_elems, const float* pos, const float* radius, const float* texcoords, const int* idx, void* vpos, float* vtex,
    void* elems, hipStream_t);
int yhk_object_lane_roots(int count, const void* rows, int shape, int root4, int root8, int root16, void* objects, hipStream_t);
// unit/refit.hip (yh_refit_shape, yh_bvh_refit_wide_gpu), all pointers DEVICE pointers unless said otherwise: the primitive boxes of a
// shape's leaf slots from new arrays (the element id is read from the record in the slot), their union as yhk_refit_partials(n) partial
// boxes, the records again in place, the boxes of one width's wide nodes level by level (level_first: HOST, levels + 1 entries; units:
// test records per primitive), and the half-area sum of a width's occupied slots as yhk_refit_partials(count) partial sums
// ... and, at a build, the levels of the three wide trees and the first wide node of each level, from the indices yhk_wide_index made
// (levels, level_first: the binary tree's, HOST; d_widx[w]: width 4 << w; d_out: 3 x 66 words of device memory; wide_levels, wide_first:
// HOST, wide_first[w][wide_levels[w]] = the count; one launch and one copy for the three widths; synchronises)
int yhk_wide_level_firsts(int num_nodes, int levels, const int* level_first, const unsigned int* const d_widx[3], unsigned int* d_out, int wide_levels[3], int wide_first[3][66],
    hipStream_t);
int yhk_refit_partials(int n);
int yhk_refit_boxes(int lines, int n, const void* recs, const float* pos, const float* radius, const int* idx, float* boxes, hipStream_t);
int yhk_box_partials(int n, const float* boxes, float* partial, hipStream_t);
int yhk_refit_records(int lines, int n, const float* pos, const float* nrm, const float* radius, const int* idx, void* recs, hipStream_t);
int yhk_refit_wide(int L, void* blob, long long node_off, long long test_off, int units, int levels, const int* level_first, const float* lboxes, hipStream_t);
int yhk_area_partials(int width, const void* blob, long long node_off, int count, double* partial, hipStream_t);
// unit/light_list.hip (yh_set_light_edits, yh_triangle_cdf_gpu), all pointers DEVICE pointers: the area cdf of every job's light from the
// scene's rows (one wave per light, the additions one float chain in element order) or of ONE job from raw positions / triangles; the
// records of the small lights among the jobs (root6: 6 floats per shape; prims: the leaf records); the coarse index of a texel cdf
int yhk_light_cdfs(int num_jobs, const void* jobs, const void* vpos, const void* elems, float* cdf, hipStream_t);
int yhk_triangle_cdf_raw(const void* job, const float* pos, const int* tri, float* cdf, hipStream_t);
int yhk_small_records(int num_jobs, const void* jobs, const float* root6, const void* prims, const float* cdf, void* table, hipStream_t);
int yhk_env_tab(int K, int S, int n, const float* cdf, float* tab, hipStream_t);
}
#endif
