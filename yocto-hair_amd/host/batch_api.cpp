// batch_api.cpp — the unit-level batch entry points of include/yhair.h (hair BSDF, intersection, BVH build, curves, self-tests).
#include "edit_internal.h"
#include "image_pass.h"  // Staged; the refusal of a scene beyond the one-lane kernels' offsets

// ---- unit-level batches ----------------------------------------------------
namespace {
int finish(yh_context* ctx, int launch_err, void* dst, const void* src, size_t bytes) {
  if (launch_err) return fail(ctx, YH_E_DEVICE, "kernel launch: %s", hipGetErrorString((hipError_t)launch_err));
  YH_WAIT(ctx);
  HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return YH_OK;
}
// the closest hits of n rays, after the wait for their kernel: object, element, uv and distance
int download_hits(yh_context* ctx, int n, const int* dob, const int* del, const float* duv, const float* dd, int* object, int* element, float* uv, float* distance) {
  HIPCHK(ctx, hipMemcpy(object, dob, 4 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(element, del, 4 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(uv, duv, 8 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(distance, dd, 4 * (size_t)n, hipMemcpyDeviceToHost));
  return YH_OK;
}
// a tree's nodes as the batch interface passes them, 8 floats each: min.xyz, max.xyz, start, num | internal << 16 | axis << 24
void pack_nodes(const yhh::Tree& tree, float* nodes) {
  for (size_t i = 0; i < tree.nodes.size(); i++) {
    auto&  nd = tree.nodes[i];
    float* o  = nodes + 8 * i;
    memcpy(o, nd.bbox.min, 12), memcpy(o + 3, nd.bbox.max, 12);
    int a = nd.start, c = (int)nd.num | ((int)nd.internal << 16) | ((int)nd.axis << 24);
    memcpy(o + 6, &a, 4), memcpy(o + 7, &c, 4);
  }
}
}  // namespace

int yh_hair_brdf_batch(yh_context* ctx, int n, const yh_material* materials, const float* v, const float* normal,
    const float* tangent, float* brdf) {
  if (!ctx || n < 0 || (n && (!materials || !v || !normal || !tangent || !brdf))) return YH_E_INVALID;
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dm = s.in(materials, sizeof(yh_material) * (size_t)n);
  auto   dv = (float*)s.in(v, 4 * (size_t)n);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   dt = (float*)s.in(tangent, 12 * (size_t)n);
  auto   o  = (float*)s.out(120 * (size_t)n);
  if (s.rc) return s.rc;
  return finish(ctx, yhk_hair_brdf(n, dm, dv, dn, dt, o, ctx->stream), brdf, o, 120 * (size_t)n);
}
static int wowi(yh_context* ctx, int n, const float* brdf, const float* a, size_t a_floats, const float* b,
    size_t b_floats, float* out, size_t out_floats, int which) {
  if (!ctx || n < 0 || (n && (!brdf || !a || !b || !out))) return YH_E_INVALID;
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   db = (float*)s.in(brdf, 120 * (size_t)n);
  auto   da = (float*)s.in(a, 4 * a_floats * n);
  auto   dbb = (float*)s.in(b, 4 * b_floats * n);
  auto   o  = (float*)s.out(4 * out_floats * n);
  if (s.rc) return s.rc;
  int e = which == 0   ? yhk_hair_eval(n, db, da, dbb, o, ctx->stream)
          : which == 1 ? yhk_hair_sample(n, db, da, dbb, o, ctx->stream)
                       : yhk_hair_pdf(n, db, da, dbb, o, ctx->stream);
  return finish(ctx, e, out, o, 4 * out_floats * n);
}
int yh_hair_eval_batch(yh_context* ctx, int n, const float* brdf, const float* wo, const float* wi, float* f) {
  return wowi(ctx, n, brdf, wo, 3, wi, 3, f, 3, 0);
}
int yh_hair_sample_batch(yh_context* ctx, int n, const float* brdf, const float* wo, const float* rn, float* wi) {
  return wowi(ctx, n, brdf, wo, 3, rn, 2, wi, 3, 1);
}
int yh_hair_pdf_batch(yh_context* ctx, int n, const float* brdf, const float* wo, const float* wi, float* pdf) {
  return wowi(ctx, n, brdf, wo, 3, wi, 3, pdf, 1, 2);
}
int yh_hair_eval_pdf_batch(yh_context* ctx, int n, const float* brdf, const float* wo, const float* wi, float* pdf) {
  return yh_hair_pdf_batch(ctx, n, brdf, wo, wi, pdf);
}

// The hair path of a shaded hit (dev_path.h: hair_setup, hair_prepare, hair_sample, the fused eval + pdf) on the material rows the upload
// makes: make_material is the upload's own code (scene_upload.cpp), so the kernels read what a render reads.
int yh_hair_shade_batch(yh_context* ctx, int form, int exact, int n, const yh_material* materials, const float* v, const float* normal,
    const float* tangent, const float* outgoing, const float* incoming, const float* rn, float* out) {
  if (!ctx || n < 0 || (form != 0 && form != 1) || (exact != 0 && exact != 1) || (exact && form != 0) ||
      (n && (!materials || !v || !normal || !tangent || !outgoing || !incoming || !rn || !out)))
    return YH_E_INVALID;
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<yhd_material> mats((size_t)n);
  for (int i = 0; i < n; i++) make_material(materials[i], mats[(size_t)i]);
  Staged s(ctx);
  auto   dm = s.in(mats.data(), sizeof(yhd_material) * (size_t)n);
  auto   dv = (float*)s.in(v, 4 * (size_t)n);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   dt = (float*)s.in(tangent, 12 * (size_t)n);
  auto   da = (float*)s.in(outgoing, 12 * (size_t)n);
  auto   db = (float*)s.in(incoming, 12 * (size_t)n);
  auto   dr = (float*)s.in(rn, 8 * (size_t)n);
  auto   o  = (float*)s.out(4 * YH_HAIR_SHADE_FLOATS * (size_t)n);
  if (s.rc) return s.rc;
  int e = exact ? yhk_hair_shade_exact(form, n, dm, dv, dn, dt, da, db, dr, o, ctx->stream)
                : yhk_hair_shade(form, n, dm, dv, dn, dt, da, db, dr, o, ctx->stream);
  return finish(ctx, e, out, o, 4 * YH_HAIR_SHADE_FLOATS * (size_t)n);
}

int yh_curves_to_lines(yh_context* ctx, int n, const float* P, const float* width0, const float* width1,
    int base_vertex, float* positions, float* normals, float* radius, int* lines) {
  if (!ctx || n < 0 || (n && (!P || !width0 || !width1 || !positions || !normals || !radius || !lines))) return YH_E_INVALID;
  if (n == 0) return YH_OK;
  if (n > 400000000 || base_vertex < 0 || (long long)base_vertex + 5ll * n > 2147483647ll)
    return fail(ctx, YH_E_INVALID, "too many curves for 32-bit vertex indices");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dp = (float*)s.in(P, 48 * (size_t)n);
  auto   d0 = (float*)s.in(width0, 4 * (size_t)n);
  auto   d1 = (float*)s.in(width1, 4 * (size_t)n);
  auto   op = (float*)s.out(60 * (size_t)n);
  auto   on = (float*)s.out(60 * (size_t)n);
  auto   orad = (float*)s.out(20 * (size_t)n);
  auto   ol = (int*)s.out(32 * (size_t)n);
  if (s.rc) return s.rc;
  int e = yhk_curves_to_lines(n, dp, d0, d1, base_vertex, op, on, orad, ol, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "k_curves_to_lines launch: %s", hipGetErrorString((hipError_t)e));
  YH_WAIT(ctx);
  HIPCHK(ctx, hipMemcpy(positions, op, 60 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(normals, on, 60 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(radius, orad, 20 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(lines, ol, 32 * (size_t)n, hipMemcpyDeviceToHost));
  return YH_OK;
}

int yh_bvh_build_gpu(yh_context* ctx, int n, const float* boxes, float* nodes, int* primitives) {
  if (!ctx || n < 0 || (n && !boxes)) return YH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<yhh::Box> b((size_t)n);
  if (n) memcpy((void*)b.data(), boxes, sizeof(yhh::Box) * (size_t)n);
  yhh::Tree tree;
  int       rc = build_bvh_device(ctx, b, tree);
  if (rc) return rc;
  if (nodes) pack_nodes(tree, nodes);
  if (primitives && n) memcpy(primitives, tree.primitives.data(), sizeof(int) * (size_t)n);
  return (int)tree.nodes.size();
}

int yh_bvh_build_wide_gpu(yh_context* ctx, int n, const float* boxes, int width, float* slots) {
  if (!ctx || n < 1 || !boxes || (width != 4 && width != 8 && width != 16)) return YH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  const int L = width == 4 ? 2 : width == 8 ? 3 : 4;
  DevBuf    d_boxes, d_nodes, d_pid, d_flag, d_widx, d_out;
  int       rc;
  if ((rc = upload(ctx, d_boxes, boxes, (size_t)n * 24))) return rc;
  if ((rc = alloc_zero(ctx, d_nodes, ((size_t)2 * n + 1) * 32)) || (rc = alloc_zero(ctx, d_pid, (size_t)n * 4))) return rc;
  int num_nodes = 0, levels = 0, level_first[130], count = 0;
  int e = yhk_bvh_build_resident(n, (const float*)d_boxes.p, (float*)d_nodes.p, (int*)d_pid.p, &num_nodes, &levels, level_first, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "device BVH build: %s", hipGetErrorString((hipError_t)e));
  if ((rc = alloc_zero(ctx, d_flag, ((size_t)num_nodes + 1) * 4)) || (rc = alloc_zero(ctx, d_widx, ((size_t)num_nodes + 1) * 4))) return rc;
  e = yhk_wide_index(num_nodes, (const float*)d_nodes.p, levels, level_first, L, (unsigned int*)d_flag.p, (unsigned int*)d_widx.p, &count, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "wide-node index: %s", hipGetErrorString((hipError_t)e));
  if (slots) {
    if ((rc = alloc_zero(ctx, d_out, (size_t)count * width * 32))) return rc;
    e = yhk_wide_collapse(L, num_nodes, (const float*)d_nodes.p, (const unsigned int*)d_flag.p, (const unsigned int*)d_widx.p, 1, 0, 0, d_out.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "wide collapse: %s", hipGetErrorString((hipError_t)e));
    YH_WAIT(ctx);
    HIPCHK(ctx, hipMemcpy(slots, d_out.p, (size_t)count * width * 32, hipMemcpyDeviceToHost));
  }
  return count;
}

int yh_bvh_build_wide(int n, const float* boxes, int width, float* slots) {
  if (n < 0 || (n && !boxes) || (width != 4 && width != 8 && width != 16)) return YH_E_INVALID;
  std::vector<yhh::Box> b((size_t)n);
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) b[(size_t)i].min[k] = boxes[6 * (size_t)i + k], b[(size_t)i].max[k] = boxes[6 * (size_t)i + 3 + k];
  yhh::Tree tree;
  yhh::build_bvh(tree, b);
  const void* data  = nullptr;
  size_t      count = 0;
  std::vector<yhh::WideNode>   w4;
  std::vector<yhh::WideNode8>  w8;
  std::vector<yhh::WideNode16> w16;
  if (width == 4) yhh::collapse_wide(tree, w4), data = w4.data(), count = w4.size();
  if (width == 8) yhh::collapse_wide8(tree, w8), data = w8.data(), count = w8.size();
  if (width == 16) yhh::collapse_wide16(tree, w16), data = w16.data(), count = w16.size();
  if (slots && count) memcpy(slots, data, count * (size_t)width * sizeof(yhh::WideSlot));
  return (int)count;
}

// what both refits check before a reference is followed, and the boxes in leaf order
static int refit_wide_args(int n, const float* boxes, const int* primitives, int width, const float* slots, std::vector<yhh::Box>& leaf_boxes, std::vector<int>& first) {
  if (n < 1 || !boxes || !primitives || !slots || (width != 4 && width != 8 && width != 16)) return YH_E_INVALID;
  static_assert(sizeof(yhh::WideSlot) == 32 && sizeof(yhh::Box) == 24, "slots and boxes are passed as floats");
  leaf_boxes.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    if (primitives[i] < 0 || primitives[i] >= n) return YH_E_INVALID;
    memcpy(&leaf_boxes[(size_t)i], boxes + 6 * (size_t)primitives[i], 24);
  }
  const int count = yhh::wide_levels(width, n, (const yhh::WideSlot*)slots, n, first);
  return count < 1 ? YH_E_INVALID : count;
}

int yh_bvh_refit_wide(int n, const float* boxes, const int* primitives, int width, float* slots) {
  std::vector<yhh::Box> leaf_boxes;
  std::vector<int>      first;
  const int             count = refit_wide_args(n, boxes, primitives, width, slots, leaf_boxes, first);
  if (count < 1) return count;
  yhh::refit_wide(width, leaf_boxes.data(), count, (yhh::WideSlot*)slots);
  return count;
}

int yh_bvh_refit_wide_gpu(yh_context* ctx, int n, const float* boxes, const int* primitives, int width, float* slots) {
  if (!ctx) return YH_E_INVALID;
  std::vector<yhh::Box> leaf_boxes;
  std::vector<int>      first;
  const int             count = refit_wide_args(n, boxes, primitives, width, slots, leaf_boxes, first);
  if (count < 1) return count < 0 ? fail(ctx, count, "yh_bvh_refit_wide_gpu: n, boxes, primitives, width or slots: no %d-wide tree over %d primitives in the device form", width, n) : count;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  YH_WAIT(ctx);
  DevBuf d_boxes, d_slots;
  int    rc;
  if ((rc = upload(ctx, d_boxes, leaf_boxes.data(), (size_t)n * 24)) || (rc = upload(ctx, d_slots, slots, (size_t)count * width * 32))) return rc;
  int e = yhk_refit_wide(width == 4 ? 2 : width == 8 ? 3 : 4, d_slots.p, 0, 0, 1, (int)first.size() - 1, first.data(), (const float*)d_boxes.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "yh_bvh_refit_wide_gpu: refit: %s", hipGetErrorString((hipError_t)e));
  YH_WAIT(ctx);
  HIPCHK(ctx, hipMemcpy(slots, d_slots.p, (size_t)count * width * 32, hipMemcpyDeviceToHost));
  return count;
}

int yh_bvh_build(int n, const float* boxes, float* nodes, int* primitives) {
  if (n < 0 || (n && !boxes)) return YH_E_INVALID;
  std::vector<yhh::Box> b((size_t)n);
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) b[(size_t)i].min[k] = boxes[6 * (size_t)i + k], b[(size_t)i].max[k] = boxes[6 * (size_t)i + 3 + k];
  yhh::Tree tree;
  yhh::build_bvh(tree, b);
  if (nodes) pack_nodes(tree, nodes);
  if (primitives && n) memcpy(primitives, tree.primitives.data(), sizeof(int) * (size_t)n);
  return (int)tree.nodes.size();
}

int yh_surface_lobe_batch(yh_context* ctx, int kind, int n, const float* params, const float* normal,
    const float* outgoing, const float* incoming, const float* rn, float* out) {
  if (!ctx || n < 0 || kind < 0 || kind >= YH_LOBE_COUNT || (n && (!params || !normal || !outgoing || !incoming || !rn || !out)))
    return YH_E_INVALID;
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dp = (float*)s.in(params, 32 * (size_t)n);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   da = (float*)s.in(outgoing, 12 * (size_t)n);
  auto   db = (float*)s.in(incoming, 12 * (size_t)n);
  auto   dr = (float*)s.in(rn, 12 * (size_t)n);
  auto   o  = (float*)s.out(28 * (size_t)n);
  if (s.rc) return s.rc;
  return finish(ctx, yhk_surface_lobe(kind, n, dp, dn, da, db, dr, o, ctx->stream), out, o, 28 * (size_t)n);
}
int yh_surface_bsdf_batch(yh_context* ctx, int n, const yh_material* materials, const float* normal,
    const float* outgoing, const float* incoming, const float* rn, float* out) {
  if (!ctx || n < 0 || (n && (!materials || !normal || !outgoing || !incoming || !rn || !out))) return YH_E_INVALID;
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<yhd_material> mats((size_t)n);
  for (int i = 0; i < n; i++) make_material(materials[i], mats[(size_t)i]);
  Staged s(ctx);
  auto   dm = s.in(mats.data(), sizeof(yhd_material) * (size_t)n);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   da = (float*)s.in(outgoing, 12 * (size_t)n);
  auto   db = (float*)s.in(incoming, 12 * (size_t)n);
  auto   dr = (float*)s.in(rn, 12 * (size_t)n);
  auto   o  = (float*)s.out(4 * YH_SURFACE_BSDF_FLOATS * (size_t)n);
  if (s.rc) return s.rc;
  return finish(ctx, yhk_surface_bsdf(n, dm, dn, da, db, dr, o, ctx->stream), out, o, 4 * YH_SURFACE_BSDF_FLOATS * (size_t)n);
}

int yh_intersect_batch(yh_context* ctx, int n, const float* rays, int* object, int* element, float* uv,
    float* distance) {
  if (!ctx || n < 0 || (n && (!rays || !object || !element || !uv || !distance))) return YH_E_INVALID;
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "yh_intersect_batch before yh_upload_scene");
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dr = (float*)s.in(rays, 32 * (size_t)n);
  auto   dob = (int*)s.out(4 * (size_t)n);
  auto   del = (int*)s.out(4 * (size_t)n);
  auto   duv = (float*)s.out(8 * (size_t)n);
  auto   dd  = (float*)s.out(4 * (size_t)n);
  if (s.rc) return s.rc;
  // Large batches of rays that start at the reference's ray_eps (every ray the path tracer itself makes) go one lane
  // per ray through the trace-only kernel (csrc/stream.hip: k_intersect_lanes), five waves per SIMD; small
  // ones, and rays with another tmin, a quad per ray (k_intersect). Same closest hits either way.
  // YHAIR_INTERSECT (developer switch): one of the two whatever the batch, and the lane kernel's waves per SIMD.
  const yhh::IntersectSwitch forced = yhh::intersect_switch();
  const int                  waves  = forced.waves;
  bool                       lanes  = n >= 65536 && lane_kernels_can_address(ctx);
  if (forced.mode == yhh::IntersectSwitch::QUAD) lanes = false;
  else if (forced.mode == yhh::IntersectSwitch::LANES) {
    if (!lane_kernels_can_address(ctx))  // (beyond 4 GB the buffer resource clamps and the loads return zeros: wrong hits, no error)
      return refuse_lane_offsets(ctx, (std::string("YHAIR_INTERSECT=") + forced.text).c_str(), "kernel");
    lanes = true;
  }
  for (int i = 0; lanes && i < n; i++) lanes = rays[8 * (size_t)i + 6] == 1e-4f;
  if (int rc = timed_begin(ctx)) return rc;
  if (lanes) {
    const int occupancy = std::min(waves, yhk_intersect_lanes_occupancy(&ctx->scene, waves));  // (256-thread blocks: one wave per SIMD each)
    if (occupancy < 1) return fail(ctx, YH_E_DEVICE, "k_intersect_lanes cannot run with its LDS layout on this device");
    const int    grid        = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n + 255) / 256, (int64_t)ctx->num_cus * occupancy));
    const int    ovf_entries = lane_overflow_entries(ctx);
    auto         dcur        = (int*)s.out(16);
    auto         dovf        = (unsigned int*)s.out((size_t)grid * 4 * ovf_entries * 64 * 4);
    if (s.rc) return s.rc;
    const yhd_scene* sc_dev = nullptr;
    if (int rc = scene_copy(ctx, &sc_dev)) return rc;
    int e = yhk_intersect_lanes(&ctx->scene, sc_dev, n, dr, dcur, dovf, ovf_entries, dob, del, duv, dd, waves, grid, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "k_intersect_lanes launch: %s", hipGetErrorString((hipError_t)e));
  } else {
    int e = yhk_intersect(&ctx->scene, n, dr, dob, del, duv, dd, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "k_intersect launch: %s", hipGetErrorString((hipError_t)e));
  }
  if (int rc = timed_end(ctx, 1)) return rc;  // (yh_last_trace_ms: the kernel alone, without the copies)
  return download_hits(ctx, n, dob, del, duv, dd, object, element, uv, distance);
}

// The lanes that own a ray in a form of yh_intersect_plain_batch; YH_E_INVALID for a form it does not have
int yh_intersect_plain_form(int form) {
  const bool in_memory = form >= 0 && (form & YH_INTERSECT_TABLE_IN_MEMORY) != 0;
  const int  base      = in_memory ? form & ~YH_INTERSECT_TABLE_IN_MEMORY : form;
  if (base < 0 || base >= YH_INTERSECT_FORMS || (in_memory && base < 3)) return YH_E_INVALID;
  return base >= 5 ? 16 : base == 1 || base >= 3 ? 8 : 4;
}

// intersect_scene_bvh through the traversal of the sample-loop kernels: forms 0 and 1 the PLAIN 512-thread ones (unit/intersect_quad.hip), forms
// 2-6 the 256-thread launch shapes and, with YH_INTERSECT_TABLE_IN_MEMORY on forms 3-6, their scene level read from memory (unit/intersect_wide.hip)
int yh_intersect_plain_batch(yh_context* ctx, int form, int n, const float* rays, int* object, int* element, float* uv, float* distance) {
  const bool in_memory = form >= 0 && (form & YH_INTERSECT_TABLE_IN_MEMORY) != 0;
  const int  base      = in_memory ? form & ~YH_INTERSECT_TABLE_IN_MEMORY : form;
  if (!ctx || n < 0 || yh_intersect_plain_form(form) < 0 || (n && (!rays || !object || !element || !uv || !distance))) return YH_E_INVALID;
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "yh_intersect_plain_batch before yh_upload_scene");
  if (!in_memory && (ctx->scene.general_materials || ctx->scene.lds_scene_f4 == 0))
    return fail(ctx, YH_E_INVALID, "yh_intersect_plain_batch: this scene renders with the GENERAL kernel variants (materials beyond diffuse / hair, a light read through memory, or tables too large for LDS)");
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dr  = (float*)s.in(rays, 32 * (size_t)n);
  auto   dob = (int*)s.out(4 * (size_t)n);
  auto   del = (int*)s.out(4 * (size_t)n);
  auto   duv = (float*)s.out(8 * (size_t)n);
  auto   dd  = (float*)s.out(4 * (size_t)n);
  if (s.rc) return s.rc;
  int e = base < 2 ? yhk_intersect_plain(&ctx->scene, base, n, dr, dob, del, duv, dd, ctx->stream)
                   : yhk_intersect_wide(&ctx->scene, base, in_memory ? 1 : 0, n, dr, dob, del, duv, dd, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s launch: %s", base < 2 ? "k_intersect_plain" : "k_intersect_wide", hipGetErrorString((hipError_t)e));
  YH_WAIT(ctx);
  return download_hits(ctx, n, dob, del, duv, dd, object, element, uv, distance);
}

int yh_scene_once(const yh_context* ctx) { return !ctx ? YH_E_INVALID : !ctx->have_scene ? YH_E_STATE : ctx->scene.scene_once; }
int yh_lights_const_env(const yh_context* ctx) { return !ctx ? YH_E_INVALID : !ctx->have_scene ? YH_E_STATE : ctx->scene.lights_const_env; }

int yh_lights_batch(yh_context* ctx, int form, int n, const float* position, const float* direction, const float* rn, float* out) {
  if (!ctx || n < 0 || (form != 0 && form != 1) || (n && (!position || !direction || !rn || !out))) return YH_E_INVALID;
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "yh_lights_batch before yh_upload_scene");
  if (n == 0) return YH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dp = (float*)s.in(position, 12 * (size_t)n);
  auto   dd = (float*)s.in(direction, 12 * (size_t)n);
  auto   dr = (float*)s.in(rn, 16 * (size_t)n);
  auto   o  = (float*)s.out(32 * (size_t)n);
  if (s.rc) return s.rc;
  if (form == 0) return finish(ctx, yhk_lights(&ctx->scene, n, dp, dd, dr, o, ctx->stream), out, o, 32 * (size_t)n);
  if (!lane_kernels_can_address(ctx)) return refuse_lane_offsets(ctx, "yh_lights_batch");
  const int ovf_entries = lane_overflow_entries(ctx);
  auto      dovf        = (unsigned int*)s.out((size_t)((n + 255) / 256) * 4 * ovf_entries * 64 * 4);
  if (s.rc) return s.rc;
  const yhd_scene* sc_dev = nullptr;
  if (int rc = scene_copy(ctx, &sc_dev)) return rc;
  return finish(ctx, yhk_lights_lanes(&ctx->scene, sc_dev, n, dp, dd, dr, dovf, ovf_entries, o, ctx->stream), out, o, 32 * (size_t)n);
}

// The homogeneous-medium code of a path (dev_path.h: medium_crossing, the free flight and the scatter of path_step) on the material rows
// the upload makes. tex 1: the row with color_tex set, so that the device derives the density from the (textured) colour and transmission.
int yh_volume_batch(yh_context* ctx, int form, int tex, int n, const yh_material* materials, const float* normal, const float* outgoing,
    const float* incoming, const float* texval, const float* rn, float* out) {
  if (!ctx || n < 1 || (form != 0 && form != 1) || (tex != 0 && tex != 1) || !materials || !normal || !outgoing || !incoming || !texval || !rn || !out)
    return YH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<yhd_material> mats((size_t)n);
  for (int i = 0; i < n; i++) {
    make_material(materials[i], mats[(size_t)i]);
    mats[(size_t)i].color_tex = tex ? 0 : -1, mats[(size_t)i].emission_tex = -1, mats[(size_t)i].scattering_tex = -1;  // (no texture is looked up: the values are given)
  }
  Staged s(ctx);
  auto   dm = s.in(mats.data(), sizeof(yhd_material) * (size_t)n);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   da = (float*)s.in(outgoing, 12 * (size_t)n);
  auto   db = (float*)s.in(incoming, 12 * (size_t)n);
  auto   dt = (float*)s.in(texval, 16 * (size_t)n);
  auto   dr = (float*)s.in(rn, 20 * (size_t)n);
  auto   ds = s.out(32 * (size_t)n);
  auto   o  = (float*)s.out(4 * YH_VOLUME_FLOATS * (size_t)n);
  if (s.rc) return s.rc;
  static const yhd_scene empty{};
  int e = form == 0 ? yhk_volume_quads(&empty, n, dm, dn, da, db, dt, dr, ds, o, ctx->stream)
                    : yhk_volume_lanes(&empty, n, dm, dn, da, db, dt, dr, ds, o, ctx->stream);
  return finish(ctx, e, out, o, 4 * YH_VOLUME_FLOATS * (size_t)n);
}

// The shading point of a hit (dev_path.h: the head of path_step / shade_step up to surface_brdf) on the uploaded scene. The loops know a hit by
// its leaf slot, the caller by its element: the leaf order of every shape the batch names is inverted on the device first (unit/point_quad.hip:
// k_point_slots), work proportional to those shapes.
int yh_point_batch(yh_context* ctx, int form, int n, const int* object, const int* element, const float* uv, const float* outgoing, float* out) {
  if (!ctx || n < 1 || form < 0 || form > 2 || !object || !element || !uv || !outgoing || !out) return YH_E_INVALID;
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "yh_point_batch before yh_upload_scene");
  const std::vector<yh_object> rows = uploaded_rows(ctx);
  const int num_objects = ctx->scene.num_objects, num_shapes = (int)ctx->lane_shapes.size();
  std::vector<int> shape_base((size_t)num_shapes, -1), shape_object((size_t)num_shapes, -1), slot_base((size_t)num_objects, 0);
  int total = 0;
  for (int i = 0; i < n; i++) {  // every index, before anything follows one
    if (object[i] < 0 || object[i] >= num_objects) return fail(ctx, YH_E_INVALID, "yh_point_batch: row %d names object %d of %d", i, object[i], num_objects);
    const int shape = rows[(size_t)object[i]].shape, num = ctx->lane_shapes[(size_t)shape].num_prims;
    if (element[i] < 0 || element[i] >= num) return fail(ctx, YH_E_INVALID, "yh_point_batch: row %d names element %d of object %d, whose shape has %d", i, element[i], object[i], num);
    if (shape_base[(size_t)shape] < 0) shape_base[(size_t)shape] = total, shape_object[(size_t)shape] = object[i], total += num;
  }
  for (int k = 0; k < num_objects; k++) slot_base[(size_t)k] = std::max(0, shape_base[(size_t)rows[(size_t)k].shape]);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dob = (int*)s.in(object, 4 * (size_t)n);
  auto   del = (int*)s.in(element, 4 * (size_t)n);
  auto   dsb = (int*)s.in(slot_base.data(), 4 * (size_t)num_objects);
  auto   duv = (float*)s.in(uv, 8 * (size_t)n);
  auto   dwo = (float*)s.in(outgoing, 12 * (size_t)n);
  auto   dso = (int*)s.out(4 * (size_t)total);
  auto   dsl = s.out(32 * (size_t)n);
  auto   o   = (float*)s.out(4 * YH_POINT_FLOATS * (size_t)n);
  if (s.rc) return s.rc;
  for (int k = 0; k < num_shapes; k++) {
    if (shape_base[(size_t)k] < 0) continue;
    int e = yhk_point_slots(&ctx->scene, shape_object[(size_t)k], ctx->lane_shapes[(size_t)k].num_prims, dso + shape_base[(size_t)k], ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "k_point_slots launch: %s", hipGetErrorString((hipError_t)e));
  }
  int e = form == 1 ? yhk_point_lanes(&ctx->scene, form, n, dob, del, dso, dsb, duv, dwo, dsl, o, ctx->stream)
                    : yhk_point_quads(&ctx->scene, form, n, dob, del, dso, dsb, duv, dwo, dsl, o, ctx->stream);
  return finish(ctx, e, out, o, 4 * YH_POINT_FLOATS * (size_t)n);
}

int yh_quad_forms_batch(yh_context* ctx, int n, const float* normal, const float* rn, const float* a, const float* b, float* out) {
  if (!ctx || n < 1 || !normal || !rn || !a || !b || !out) return YH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staged s(ctx);
  auto   dn = (float*)s.in(normal, 12 * (size_t)n);
  auto   dr = (float*)s.in(rn, 8 * (size_t)n);
  auto   da = (float*)s.in(a, 12 * (size_t)n);
  auto   db = (float*)s.in(b, 4 * (size_t)n);
  auto   o  = (float*)s.out(4 * YH_QUAD_FORMS_FLOATS * (size_t)n);
  if (s.rc) return s.rc;
  return finish(ctx, yhk_quad_forms(n, dn, dr, da, db, o, ctx->stream), out, o, 4 * YH_QUAD_FORMS_FLOATS * (size_t)n);
}

// The start and the end of a path (dev_path.h: path_begin with sample_camera / sample_camera_lane, path_continue, path_end), row by row.
int yh_path_ends_batch(yh_context* ctx, int op, int form, int n, const float* fin, const int* iin, const uint64_t* rng, float* fout, int* iout,
    uint64_t* state) {
  if (!ctx || n < 1 || op < 0 || op >= YH_PATH_OPS || (form != 0 && form != 1) || !fin || !iin || !fout) return YH_E_INVALID;
  const bool draws = op != YH_PATH_END;  // (path_end draws nothing and returns no ints)
  if (draws && (!rng || !iout || !state)) return YH_E_INVALID;
  static const size_t floats_in[YH_PATH_OPS] = {YH_PATH_BEGIN_IN, YH_PATH_CONTINUE_IN, YH_PATH_END_IN}, ints_in[YH_PATH_OPS] = {4, 2, 1};
  static const size_t floats_out[YH_PATH_OPS] = {YH_PATH_BEGIN_OUT, YH_PATH_CONTINUE_OUT, YH_PATH_END_OUT}, ints_out[YH_PATH_OPS] = {3, 2, 0};
  static_assert(sizeof(yhd_camera) == 4 * YH_PATH_BEGIN_IN, "a row of YH_PATH_BEGIN is the kernels' camera");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t rows = (size_t)n;
  Staged s(ctx);
  auto   df = (float*)s.in(fin, 4 * floats_in[op] * rows);
  auto   di = (int*)s.in(iin, 4 * ints_in[op] * rows);
  auto   dr = draws ? (uint64_t*)s.in(rng, 16 * rows) : nullptr;
  auto   of = (float*)s.out(4 * floats_out[op] * rows);
  auto   oi = draws ? (int*)s.out(4 * ints_out[op] * rows) : nullptr;
  auto   os = draws ? (uint64_t*)s.out(8 * rows) : nullptr;
  if (s.rc) return s.rc;
  int e = form == 0 ? yhk_path_ends_quads(op, n, df, di, dr, of, oi, os, ctx->stream) : yhk_path_ends_lanes(op, n, df, di, dr, of, oi, os, ctx->stream);
  if (int rc = finish(ctx, e, fout, of, 4 * floats_out[op] * rows)) return rc;
  if (!draws) return YH_OK;
  HIPCHK(ctx, hipMemcpy(iout, oi, 4 * ints_out[op] * rows, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(state, os, 8 * rows, hipMemcpyDeviceToHost));
  return YH_OK;
}

// ---- the four self-tests (ext.cpp:555-693) ---------------------------------
// The host replays the reference's serial structure (seed, loop bounds with
// the accumulating float counters, per-block draw counts) and hands every
// (beta_m, beta_n) block to the device with the generator state at its start.
int yh_selftest(yh_context* ctx, int which, float* worst) {
  if (!ctx) return YH_E_INVALID;
  if (which < 0 || which > 3) return fail(ctx, YH_E_INVALID, "unknown self-test %d", which);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf sums, wbits;
  int    rc;
  if ((rc = alloc_zero(ctx, sums, 6 * sizeof(double)))) return rc;
  if ((rc = alloc_zero(ctx, wbits, 4))) return rc;
  auto lum = [](const double* s) { return (float)(0.2126 * s[0] + 0.7152 * s[1] + 0.0722 * s[2]); };
  auto sample_sphere = [](float rx, float ry, float* w) {  // math.h:4847-4852
    float z = 2 * ry - 1;
    float r = std::sqrt(fmin_(fmax_(1 - z * z, 0.0f), 1.0f));
    float phi = 2 * pif * rx;
    w[0] = r * std::cos(phi), w[1] = r * std::sin(phi), w[2] = z;
  };
  Rng   rng = make_rng(199382389514ULL);
  float wo[3] = {0, 0, 1};
  if (which == 0 || which == 1) {
    float x = rand1f(rng), y = rand1f(rng);
    sample_sphere(x, y, wo);
  }
  bool  ok  = true;
  float dev = 0;
  auto run = [&](float bm, float bn, int count, int per_iter, double* out, float* dmax) -> int {
    HIPCHK(ctx, hipMemsetAsync(sums.p, 0, 6 * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(wbits.p, 0, 4, ctx->stream));
    int e = yhk_selftest(which, bm, bn, rng.state, rng.inc, count, wo, (double*)sums.p, (unsigned int*)wbits.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "k_selftest launch: %s", hipGetErrorString((hipError_t)e));
    YH_WAIT(ctx);
    HIPCHK(ctx, hipMemcpy(out, sums.p, 6 * sizeof(double), hipMemcpyDeviceToHost));
    unsigned int bits;
    HIPCHK(ctx, hipMemcpy(&bits, wbits.p, 4, hipMemcpyDeviceToHost));
    memcpy(dmax, &bits, 4);
    skip_rng(rng, (uint64_t)count * per_iter);
    return YH_OK;
  };
  double s[6];
  float  d;
  if (which == 0 || which == 1) {
    for (float bm = 0.1f; bm < 1.0f; bm += 0.2f)
      for (float bn = 0.1f; bn < 1.0f; bn += 0.2f) {
        const int count = 300000;
        if ((rc = run(bm, bn, count, 3, s, &d))) return rc;
        float avg = which == 0 ? lum(s) / (count * (1 / (4 * pif))) : lum(s) / count;
        float lo = which == 0 ? 0.95f : 0.99f, hi = which == 0 ? 1.05f : 1.01f;
        if (!(avg >= lo && avg <= hi)) ok = false;
        dev = fmax_(dev, std::fabs(avg - 1));
      }
  } else if (which == 2) {
    for (float bm = 0.1f; bm < 1.0f; bm += 0.2f)
      for (float bn = 0.4f; bn < 1.0f; bn += 0.2f) {
        if ((rc = run(bm, bn, 10000, 5, s, &d))) return rc;
        if (!(d <= 0.001f)) ok = false;
        dev = fmax_(dev, d);
      }
  } else {
    for (float bm = 0.2f; bm < 1.0f; bm += 0.2f)
      for (float bn = 0.4f; bn < 1.0f; bn += 0.2f) {
        const int count = 64 * 1024;
        float x = rand1f(rng), y = rand1f(rng);
        sample_sphere(x, y, wo);
        if ((rc = run(bm, bn, count, 3, s, &d))) return rc;
        float fi = lum(s) / count, fu = lum(s + 3) / (count * (1 / (4 * pif)));
        float err = std::fabs(fi - fu) / fu;
        if (err >= 0.05f) ok = false;
        dev = fmax_(dev, err);
      }
  }
  if (worst) *worst = dev;
  if (!ok) return fail(ctx, YH_E_SELFTEST, "TEST FAILED! (self-test %d, worst deviation %g)", which, dev);
  return YH_OK;
}
