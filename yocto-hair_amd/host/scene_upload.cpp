// scene_upload.cpp — yh_upload_scene = init_bvh + init_lights (pt.cpp:755-818,1695-1740): everything a launch reads is made here, big shapes
// entirely on the device (csrc/bvh_gpu.hip); nothing is deferred to a first launch (rounds 3-5 built the 8- / 16-wide nodes there).
#include "edit_internal.h"  // SceneLevelStage, and the rules the upload shares with the edits

#include <atomic>

// The material-only part of eval_hair_brdf (ext.cpp:131-172) plus the
// per-lobe constants the kernels use (dev_hair.h). Same libm as the reference
// (this runs on the host), so these values are bit-identical to what the
// reference recomputes at every hit.
void make_material(const yh_material& m, yhd_material& d) {
  memset(&d, 0, sizeof(d));
  memcpy(d.emission, m.emission, 12);
  memcpy(d.color, m.color, 12);
  float dmax    = fmax_(fmax_(m.color[0], m.color[1]), m.color[2]);
  d.diffuse_pdf = dmax ? dmax / dmax : 0.0f;  // pt.cpp:456-471 with one lobe
  d.thin        = m.thin;
  d.specular = m.specular, d.metallic = m.metallic, d.roughness = m.roughness, d.ior = m.ior;
  d.transmission = m.transmission;
  d.opacity      = m.opacity * ((1.0f + 1.0f + 1.0f) / 3);  // mean of the {1,1,1} null texture (pt.cpp:425)
  if (d.opacity > 0.999f) d.opacity = 1;
  d.emission_tex = m.emission_tex - 1, d.color_tex = m.color_tex - 1, d.scattering_tex = m.scattering_tex - 1;
  d.trdepth = m.trdepth;
  d.plain = m.specular == 0 && m.metallic == 0 && m.transmission == 0 && d.opacity == 1 && m.emission_tex == 0 &&
            m.color_tex == 0 && m.scattering_tex == 0;
  for (int c = 0; c < 3; c++) {  // reflectivity_to_eta (math.h:4270-4273)
    float r   = fmin_(fmax_(m.color[c], 0.0f), 0.99f);
    d.meta[c] = (1 + std::sqrt(r)) / (1 - std::sqrt(r));
  }
  d.has_volume = !m.thin && m.transmission != 0;
  for (int c = 0; c < 3; c++) {  // eval_vsdf (pt.cpp:520-524)
    d.vol_density[c] = d.has_volume ? -std::log(fmin_(fmax_(m.color[c], 0.0001f), 1.0f)) / m.trdepth : 0.0f;
    d.vol_scatter[c] = m.scattering[c];
  }
  d.vol_anisotropy = m.scanisotropy;
  F3 sa{0, 0, 0};
  if (m.sigma_a[0] || m.sigma_a[1] || m.sigma_a[2]) {
    sa = ld3(m.sigma_a);
  } else if (m.color[0] || m.color[1] || m.color[2]) {  // ext.cpp:121-125
    float bn  = m.beta_n;
    float den = 5.969f - 0.215f * bn + 2.532f * sqr(bn) - 10.73f * powt<3>(bn) + 5.574f * powt<4>(bn) +
                0.245f * powt<5>(bn);
    F3 q = {std::log(m.color[0]) / den, std::log(m.color[1]) / den, std::log(m.color[2]) / den};
    sa   = {q.x * q.x, q.y * q.y, q.z * q.z};
  } else if (m.eumelanin || m.pheomelanin) {  // ext.cpp:115-119
    F3 e = F3{0.419f, 0.697f, 1.37f}, p = F3{0.187f, 0.4f, 1.05f};
    sa   = F3{m.eumelanin * e.x, m.eumelanin * e.y, m.eumelanin * e.z} +
         F3{m.pheomelanin * p.x, m.pheomelanin * p.y, m.pheomelanin * p.z};
  }
  st3(d.sigma_a, sa);
  d.alpha = m.alpha, d.eta = m.eta;
  float bm = m.beta_m, bn = m.beta_n;
  d.v[0] = sqr(0.726f * bm + 0.812f * sqr(bm) + 3.7f * powt<20>(bm));
  d.v[1] = 0.25f * d.v[0];
  d.v[2] = 4 * d.v[0];
  d.v[3] = d.v[2];
  d.s    = 0.626657069f * (0.265f * bn + 1.194f * sqr(bn) + 5.372f * powt<22>(bn));
  d.sin_2k_alpha[0] = std::sin(pif / 180 * d.alpha);
  d.cos_2k_alpha[0] = std::sqrt(fmax_(0.0f, 1 - sqr(d.sin_2k_alpha[0])));
  for (int i = 1; i < 3; i++) {
    d.sin_2k_alpha[i] = 2 * d.cos_2k_alpha[i - 1] * d.sin_2k_alpha[i - 1];
    d.cos_2k_alpha[i] = sqr(d.cos_2k_alpha[i - 1]) - sqr(d.sin_2k_alpha[i - 1]);
  }
  for (int p = 0; p < 4; p++) {
    d.inv_v[p]        = 1 / d.v[p];
    d.log_inv_2v[p]   = std::log(1 / (2 * d.v[p]));
    d.exp_m2_inv_v[p] = std::exp(-2 / d.v[p]);
    d.mp_den[p]       = ::sinh((double)(1 / d.v[p])) * 2 * d.v[p];
  }
  float cb   = 1 / (1 + std::exp(-pif / d.s));
  float ca   = 1 / (1 + std::exp(-(-pif) / d.s));
  d.tl_cdf_a = ca;
  d.tl_norm  = cb - ca;
}


// The maps of a material that change its pixels: all but transmission_tex (pt.cpp:421-422 reads emission_tex instead).
static bool has_effective_map(const yh_material_maps& m) {
  return m.specular_tex || m.metallic_tex || m.roughness_tex || m.opacity_tex || m.normal_tex;
}

static_assert(sizeof(yhd_maps) == 32, "yhd_maps");

// The material section of the upload, which yh_update_materials runs again for the rows it replaces (scene_edit.cpp).
bool make_material_rows(const yh_material* materials, const yh_material_maps* maps, int count, yhd_material* rows, yhd_maps* dmaps) {
  bool general = false;
  for (int i = 0; i < count; i++) {
    make_material(materials[i], rows[i]);
    if (maps) {  // the lookups and the lobe set-up of a mapped material happen per hit (dev_path.h: eval_hit_maps)
      const yh_material_maps& m = maps[i];
      yhd_maps&               d = dmaps[i];
      d.specular_tex = m.specular_tex - 1, d.metallic_tex = m.metallic_tex - 1, d.roughness_tex = m.roughness_tex - 1;
      d.opacity_tex = m.opacity_tex - 1, d.normal_tex = m.normal_tex - 1;
      d.any = has_effective_map(m) ? 1 : 0, d.opacity = materials[i].opacity, d.pad = 0;
      if (d.any) rows[i].plain = 0;
    }
    if (!rows[i].plain) general = true;
  }
  return general;
}

// Which kernel variant a scene table runs, once its materials are known (`general_rows`: one of them is not plain), and whether the plain
// 512-thread kernels resolve its scene level once per ray.
void settle_scene_variant(const yh_context* ctx, yhd_scene& sc, bool general_rows) {
  // a light sampled and intersected through memory: the general kernel variant (dev_path.h: BIG_LIGHTS); the plain variants rely on the
  // material table and on the scene-level table in LDS (dev_path.h)
  sc.general_materials = general_rows || ctx->big_lights || sc.lds_materials == 0 || sc.lds_scene_f4 == 0;
  // THE SCENE LEVEL ONCE PER RAY (csrc/dev_trace.h: ONCE): a plain scene whose scene level is one leaf node. Its records (8 KB per
  // object in the 512-thread quad form) must cost shapes 0 and 5 no resident workgroup, else the scene keeps the in-loop form
  sc.scene_once = 0;
  if (!sc.general_materials && sc.num_scene_nodes == 1 && sc.num_objects >= 1 && sc.num_objects <= 4) {
    const int quad0 = yhk_trace_occupancy(yhk_trace_lds_bytes(&sc, YH_SHAPE_QUAD), 0, YH_SHAPE_QUAD);
    const int sbs0  = yhk_trace_sbs_occupancy(yhk_trace_sbs_lds_bytes(&sc), 0);
    sc.scene_once = sc.num_objects;
    if (yhk_trace_occupancy(yhk_trace_lds_bytes(&sc, YH_SHAPE_QUAD), 0, YH_SHAPE_QUAD) < quad0 || yhk_trace_sbs_occupancy(yhk_trace_sbs_lds_bytes(&sc), 0) < sbs0)
      sc.scene_once = 0;
  }
  // LIGHTS THAT ARE CONSTANT ENVIRONMENTS ONLY (csrc/dev_path.h: CENV): a plain scene none of whose environments has a texture and none of
  // whose lights is an object. From the table as it stands: every edit that makes the light list again comes through here afterwards.
  sc.lights_const_env = sc.general_materials ? 0 : 1;
  for (int ei = 0; ei < sc.num_environments; ei++)
    if (sc.environments[ei].tex_w != 0 || sc.environments[ei].tex_h != 0) sc.lights_const_env = 0;
  for (int li = 0; li < sc.num_lights; li++)
    if (sc.lights[li].object >= 0 || sc.lights[li].environment < 0) sc.lights_const_env = 0;
}

// Fingerprint of the scene for the process-wide trial record: counts, camera, materials, objects, a sample of the geometry, environment
// heads, maps — over the bytes the context keeps of them, so that an edited scene has the key an upload of the edited description computes.
uint64_t scene_fingerprint(const yh_context* ctx) {
  uint64_t h = 1469598103934665603ULL;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ULL;
  };
  mix(&ctx->key_camera, sizeof(ctx->key_camera));
  mix(ctx->h_materials.data(), sizeof(yh_material) * ctx->h_materials.size());
  mix(ctx->key_geometry.data(), ctx->key_geometry.size());
  mix(ctx->key_envs.data(), ctx->key_envs.size());
  mix(ctx->h_maps.data(), sizeof(yh_material_maps) * ctx->h_maps.size());
  return h;
}

// A new scene, or an edited one: no image state, no measured costs, nothing planned; the streaming kernel's copy of the scene table is
// made again at its first launch (stream_impl).
void forget_image_of_scene(yh_context* ctx) {
  ctx->d_scene_copy.reset();
  ctx->have_state = false;
  ctx->launch_shape = YH_SHAPE_QUAD;
  ctx->item_cost.clear();
  ctx->have_costs = false, ctx->costs_settled = false, ctx->dense = -1, ctx->chain = -1, ctx->chain16 = -1;
  for (double& t : ctx->shape_ms) t = 0;
  for (int& t : ctx->shape_trials) t = 0;
  ctx->trials_from_disk = false;
}

// The levels of a host-built tree as the device builder reports them: their number and the first node of each (level_first[0 .. levels],
// 130 entries). false: more than 128 levels.
bool tree_levels(const yhh::Tree& tree, int& levels, int* level_first) {
  std::vector<int> level(tree.nodes.size(), 0);
  for (size_t n = 0; n < tree.nodes.size(); n++)
    if (tree.nodes[n].internal) level[(size_t)tree.nodes[n].start] = level[(size_t)tree.nodes[n].start + 1] = level[n] + 1;
  const int num_nodes = (int)tree.nodes.size();
  levels = level.empty() ? 1 : level.back() + 1;  // (breadth-first numbering: levels are contiguous, the last node is on the last one)
  if (levels > 128) return false;
  for (int l = 0; l <= levels; l++) level_first[l] = num_nodes;
  for (size_t n = tree.nodes.size(); n-- > 0;) level_first[level[n]] = (int)n;
  return true;
}

// The index of the 4-wide nodes of a scene tree that is walked out of the lane blob (the upload, and every edit that builds the tree
// again): the binary nodes on the device and, per node, the flag and the index of its wide node, for yhk_wide_collapse.
int index_scene_tree(yh_context* ctx, const char* who, const yhh::Tree& tree, DevBuf& d_stree, DevBuf& d_sflag, DevBuf& d_sidx, int* wide_count, int* wide_depth) {
  const int nn = (int)tree.nodes.size();
  int levels = 1, level_first[130] = {0};
  if (!tree_levels(tree, levels, level_first)) return fail(ctx, YH_E_INVALID, "%sscene tree of %d levels", who, levels);
  if (int rc = dev_alloc(ctx, d_stree, (size_t)nn * 32)) return rc;
  if (int rc = dev_alloc(ctx, d_sflag, ((size_t)nn + 1) * 4)) return rc;
  if (int rc = dev_alloc(ctx, d_sidx, ((size_t)nn + 1) * 4)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(d_stree.p, tree.nodes.data(), (size_t)nn * 32, hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_wide_index(nn, (const float*)d_stree.p, levels, level_first, 2, (unsigned int*)d_sflag.p, (unsigned int*)d_sidx.p, wide_count, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "wide-node index of the scene tree: %s", hipGetErrorString((hipError_t)e));
  *wide_depth = 1 + std::max(0, levels - 2) / 2;
  return YH_OK;
}

// scene-level LDS table: objects (YH_OBJECT_F4 = 11 float4 each), scene BVH nodes (2 float4 each), primitive ids; up to 10 KB = 46
// objects. A scene with more runs the GENERAL kernel variants, which read the table from memory, and walks its scene level as 4-wide
// nodes out of the blob (an instanced scene has thousands of objects)
static bool scene_level_is_wide(int num_objects, int num_scene_nodes, int* lds_scene_f4) {
  static_assert(sizeof(yhd_object) == 16 * YH_OBJECT_F4, "yhd_object is staged to LDS as float4");
  *lds_scene_f4 = YH_OBJECT_F4 * num_objects + 2 * num_scene_nodes + (num_objects + 3) / 4;
  return *lds_scene_f4 * 16 > 10240;
}

// a wide node pushes at most three entries and keeps the fourth in a register; the scene level: a binary node pushes one, a leaf up to three
// objects — or, walked as 4-wide nodes, three per node and the leaf's three (the same quad form under every launch shape). An 8-wide node
// pushes at most seven, a 16-wide one fifteen
static StackNeeds stack_needs(bool scene_wide, int scene_wide_depth, int scene_tree_depth, int depth4, int depth8, int depth16) {
  const int scene_need = scene_wide ? 3 * scene_wide_depth + 4 : scene_tree_depth + 4;
  return {scene_need + 3 * depth4 + 2, scene_need + 7 * depth8 + 2, scene_need + 15 * depth16 + 2};
}

// Everything the scene level is, from every object's world box and the deepest shape tree per width (edit_internal.h): the reference's
// tree, whether it is walked as 4-wide nodes and their index if so, the stack needs, and the two arrays the kernels stage to LDS.
int derive_scene_level(yh_context* ctx, const char* who, const std::vector<yhh::Box>& boxes, int num_objects, int depth4, int depth8, int depth16, SceneLevelStage& S) {
  yhh::build_bvh(S.tree, boxes);
  S.nn         = (int)S.tree.nodes.size();
  S.scene_wide = scene_level_is_wide(num_objects, S.nn, &S.lds_scene_f4);
  if (S.scene_wide)
    if (int rc = index_scene_tree(ctx, who, S.tree, S.d_stree, S.d_sflag, S.d_sidx, &S.wide_count, &S.wide_depth)) return rc;
  S.needs = stack_needs(S.scene_wide, S.wide_depth, S.tree.max_depth, depth4, depth8, depth16);
  for (auto& n : S.tree.nodes) S.scene_nodes.push_back(node_lo(n)), S.scene_nodes.push_back(node_hi(n));  // (binary, also of a scene walked through its wide nodes: the counted builds' yardstick)
  S.scene_prims = S.tree.primitives;
  S.scene_prims.resize((S.scene_prims.size() + 3) / 4 * 4, 0);  // staged to LDS as float4
  return YH_OK;
}
int check_stack_needs(yh_context* ctx, const char* who, const StackNeeds& needs) {
  if (needs.need > yhk_stack_entries()) return fail(ctx, YH_E_INVALID, "%sBVH too deep for the traversal stack (%d > %d)", who, needs.need, yhk_stack_entries());
  return YH_OK;
}
// ... its 4-wide nodes into the front of the traversal array `blob`: leaf references as of a line shape whose test records start at 0,
// count << 27 | first scene primitive
int collapse_scene_tree(yh_context* ctx, const SceneLevelStage& S, void* blob) {
  if (!S.scene_wide) return YH_OK;
  int e = yhk_wide_collapse(2, S.nn, (const float*)S.d_stree.p, (const unsigned int*)S.d_sflag.p, (const unsigned int*)S.d_sidx.p, 1, 0, 0, blob, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "wide collapse of the scene tree: %s", hipGetErrorString((hipError_t)e));
  return YH_OK;
}
// ... and its fields of a scene table whose two arrays are in the context's buffers, with the three stack sizes
void set_scene_level_fields(yh_context* ctx, yhd_scene& sc, const SceneLevelStage& S) {
  ctx->stack_need = S.needs.need, ctx->stack_need8 = S.needs.need8, ctx->stack_need16 = S.needs.need16;
  sc.scene_nodes = (const yhd_float4*)ctx->d_scene_nodes.p, sc.scene_prims = (const int*)ctx->d_scene_prims.p;
  sc.num_scene_nodes = S.nn;
  sc.lds_scene_f4    = S.scene_wide ? 0 : S.lds_scene_f4;
  sc.scene_wide_root = S.scene_wide ? 0 : -1;
  auto entries = [](int need) { return std::max(8, (need + 7) / 8 * 8); };
  sc.stack_entries = entries(S.needs.need), sc.stack_entries8 = entries(S.needs.need8), sc.stack_entries16 = entries(S.needs.need16);
}

// ---- one shape's tree and leaf-ordered records: what the upload runs per shape and yh_update_shape for the one it edits ----------------
// BIG shapes (>= 32 768 primitives: the hair) never leave the device (round 6): their vertex arrays cross PCIe once, as they are, and
// bounds, the reference's tree (csrc/bvh_gpu.hip), the leaf-ordered records and the wide collapses are made there. SMALL shapes
// (the configs' sphere and lights: 10 ms together) are built on the host and their trees and records uploaded into the same arrays;
// the collapses are the device's for both. YHAIR_BVH=host: every shape the small way; YHAIR_BVH=device: every shape on the device.
bool shape_builds_on_device(int num_prims) {
  const yhh::BvhSwitch forced = yhh::bvh_switch();
  return (num_prims >= 32768 || forced == yhh::BVH_DEVICE) && forced != yhh::BVH_HOST;
}

// `s`: the shape, its indices checked; its arrays on the host, or (arrays_on_device, which needs on_device) in device memory. The records
// go to d_recs (device: 4 float4 per segment, 6 per triangle), the binary tree to T.d_tree; `who` begins every message ("" for the upload).
int build_shape_tree(yh_context* ctx, const char* who, int si, const yh_shape& s, bool arrays_on_device, bool on_device, yhd_float4* d_recs, ShapeTree& T) {
  const bool lines = s.num_lines > 0;
  const int  nel   = lines ? s.num_lines : s.num_triangles;
  const int* idx   = lines ? s.lines : s.triangles;
  int        rc;
  T.kind = lines ? YH_KIND_LINES : YH_KIND_TRIANGLES, T.num_prims = nel;
  T.host_prims.clear();
  if (on_device) {
    // ---- on the device ----
    const size_t nv = (size_t)s.num_vertices;
    DevBuf d_pos, d_nrm, d_rad, d_idx, d_boxes, d_pid;
    const void *p_pos = s.positions, *p_nrm = s.normals, *p_rad = s.radius, *p_idx = idx;
    auto h2d = [&](DevBuf& buf, const void*& src, size_t bytes) -> int {
      if (arrays_on_device) return YH_OK;
      if (int arc = dev_alloc(ctx, buf, bytes)) return arc;
      HIPCHK(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
      src = buf.p;
      return YH_OK;
    };
    if ((rc = h2d(d_pos, p_pos, nv * 12))) return rc;
    if (s.radius && (rc = h2d(d_rad, p_rad, nv * 4))) return rc;
    if ((rc = h2d(d_idx, p_idx, (size_t)nel * (lines ? 8 : 12)))) return rc;
    if ((rc = dev_alloc(ctx, d_boxes, (size_t)nel * 24))) return rc;
    if ((rc = dev_alloc(ctx, d_pid, (size_t)nel * 4))) return rc;
    if ((rc = dev_alloc(ctx, T.d_tree, ((size_t)2 * nel + 1) * 32))) return rc;
    int e = yhk_prim_boxes(lines ? 1 : 0, nel, (const float*)p_pos, (const float*)p_rad, (const int*)p_idx, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sprimitive bounds: %s", who, hipGetErrorString((hipError_t)e));
    // (the normals' copy is queued behind the kernels that do not need it: it travels while the tree is built)
    if (s.normals && (rc = h2d(d_nrm, p_nrm, nv * 12))) return rc;
    e = yhk_bvh_build_resident(nel, (const float*)d_boxes.p, (float*)T.d_tree.p, (int*)d_pid.p, &T.num_nodes, &T.levels, T.level_first, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sdevice BVH build: %s", who, hipGetErrorString((hipError_t)e));
    e = yhk_leaf_records(lines ? 1 : 0, nel, (const int*)d_pid.p, (const float*)p_pos, (const float*)p_nrm, (const float*)p_rad, (const int*)p_idx, d_recs, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sleaf records: %s", who, hipGetErrorString((hipError_t)e));
    float root8[8];
    HIPCHK(ctx, hipMemcpyAsync(root8, T.d_tree.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    YH_WAIT(ctx);  // (the vertex arrays go out of scope)
    memcpy(T.root.min, root8, 12), memcpy(T.root.max, root8 + 3, 12);
  } else {
    // ---- on the host (small shapes) ----
    auto pos = [&](int v) { return ld3(s.positions + 3 * (size_t)v); };
    auto rad = [&](int v) { return s.radius ? s.radius[v] : 0.001f; };  // add_radius, sceneio.cpp:390
    std::vector<yhh::Box> boxes(nel);
    parallel_for(nel, [&](int e) {
      if (lines) {  // line_bounds (math.h:3037-3040)
        int a = idx[2 * e], b = idx[2 * e + 1];
        F3  p0 = pos(a), p1 = pos(b);
        float r0 = rad(a), r1 = rad(b);
        float lo0[3] = {p0.x - r0, p0.y - r0, p0.z - r0}, lo1[3] = {p1.x - r1, p1.y - r1, p1.z - r1};
        float hi0[3] = {p0.x + r0, p0.y + r0, p0.z + r0}, hi1[3] = {p1.x + r1, p1.y + r1, p1.z + r1};
        for (int k = 0; k < 3; k++) boxes[e].min[k] = fmin_(lo0[k], lo1[k]), boxes[e].max[k] = fmax_(hi0[k], hi1[k]);
      } else {  // triangle_bounds (math.h:3041-3044)
        const float* p0 = s.positions + 3 * (size_t)idx[3 * e];
        const float* p1 = s.positions + 3 * (size_t)idx[3 * e + 1];
        const float* p2 = s.positions + 3 * (size_t)idx[3 * e + 2];
        for (int k = 0; k < 3; k++) {
          boxes[e].min[k] = fmin_(p0[k], fmin_(p1[k], p2[k]));
          boxes[e].max[k] = fmax_(p0[k], fmax_(p1[k], p2[k]));
        }
      }
    });
    yhh::Tree tree;
    yhh::build_bvh(tree, boxes);
    // the tree as the device builder leaves it: 8 floats per node (yhh::Node has that layout byte for byte), the first node of every level
    static_assert(sizeof(yhh::Node) == 32 && offsetof(yhh::Node, start) == 24 && offsetof(yhh::Node, num) == 28 && offsetof(yhh::Node, internal) == 30 && offsetof(yhh::Node, axis) == 31,
        "yhh::Node is the device's node record");
    T.num_nodes = (int)tree.nodes.size();
    if (!tree_levels(tree, T.levels, T.level_first)) return fail(ctx, YH_E_INVALID, "%sshape %d: tree of %d levels", who, si, T.levels);
    if ((rc = upload(ctx, T.d_tree, tree.nodes.data(), tree.nodes.size() * 32))) return rc;
    T.root = tree.nodes[0].bbox;
    auto nrm = [&](int v) { return s.normals ? ld3(s.normals + 3 * (size_t)v) : F3{0, 0, 0}; };
    const size_t per = lines ? 4 : 6;
    T.host_prims.resize(per * (size_t)nel);
    yhd_float4* out = T.host_prims.data();
    parallel_for(nel, [&](int slot) {
      int   e = tree.primitives[slot];
      float ew;
      memcpy(&ew, &e, 4);
      yhd_float4* r = out + per * (size_t)slot;
      if (lines) {
        int a = idx[2 * e], b = idx[2 * e + 1];
        F3  p0 = pos(a), p1 = pos(b), t0 = nrm(a), t1 = nrm(b);
        r[0] = {p0.x, p0.y, p0.z, rad(a)}, r[1] = {p1.x, p1.y, p1.z, rad(b)};
        r[2] = {t0.x, t0.y, t0.z, ew}, r[3] = {t1.x, t1.y, t1.z, 0};
      } else {
        int a = idx[3 * e], b = idx[3 * e + 1], cc = idx[3 * e + 2];
        F3  p0 = pos(a), p1 = pos(b), p2 = pos(cc), n0 = nrm(a), n1 = nrm(b), n2 = nrm(cc);
        r[0] = {p0.x, p0.y, p0.z, ew}, r[1] = {p1.x, p1.y, p1.z, 0}, r[2] = {p2.x, p2.y, p2.z, 0};
        r[3] = {n0.x, n0.y, n0.z, 0}, r[4] = {n1.x, n1.y, n1.z, 0}, r[5] = {n2.x, n2.y, n2.z, 0};
      }
    });
    HIPCHK(ctx, hipMemcpy(d_recs, T.host_prims.data(), T.host_prims.size() * 16, hipMemcpyHostToDevice));
  }
  {  // depths of the wide trees: a W-wide node stands for every internal binary node at a level that is a multiple of log2 W, so the wide
     // depth is 1 + deepest internal level / log2 W (what collapse_wide / _wide8 / _wide16 return). The last level holds leaves only.
    const int deepest = std::max(0, T.levels - 2);
    T.depth = 1 + deepest / 2, T.depth8 = 1 + deepest / 3, T.depth16 = 1 + deepest / 4;
  }
  return YH_OK;
}

// The index of every 4- / 8- / 16-wide node of a built tree (one flag pass + one scan per width) and their counts.
int index_shape_tree(yh_context* ctx, const char* who, ShapeTree& T) {
  for (int w = 0; w < 3; w++) {
    if (int rc = dev_alloc(ctx, T.d_wflag[w], ((size_t)T.num_nodes + 1) * 4)) return rc;
    if (int rc = dev_alloc(ctx, T.d_widx[w], ((size_t)T.num_nodes + 1) * 4)) return rc;
    int e = yhk_wide_index(T.num_nodes, (const float*)T.d_tree.p, T.levels, T.level_first, 2 + w, (unsigned int*)T.d_wflag[w].p, (unsigned int*)T.d_widx[w].p, &T.wide_count[w], ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%swide-node index: %s", who, hipGetErrorString((hipError_t)e));
  }
  // the first wide node of every level of the three wide trees, for a later refit (unit/refit.hip): the scans' values at the levels' first nodes
  DevBuf d_firsts;
  if (int rc = dev_alloc(ctx, d_firsts, 3 * 66 * 4)) return rc;
  const unsigned int* widx[3] = {(const unsigned int*)T.d_widx[0].p, (const unsigned int*)T.d_widx[1].p, (const unsigned int*)T.d_widx[2].p};
  int e = yhk_wide_level_firsts(T.num_nodes, T.levels, T.level_first, widx, (unsigned int*)d_firsts.p, T.wide_levels, T.wide_first, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%swide-node levels: %s", who, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

// ... and the nodes themselves with the shape's test records, into the traversal array `blob` (the context's, or the grown copy an edit swaps in)
int collapse_shape_tree(yh_context* ctx, const char* who, const ShapeTree& T, const yh_context::LaneShape& L, void* blob) {
  int e = yhk_lane_tests((const yhd_float4*)ctx->d_prims.p, (yhd_float4*)blob, L.kind, L.prim_base, L.num_prims, L.test_off, ctx->stream);
  const long long offs[3] = {L.node_off, L.node_off8, L.node_off16};
  for (int w = 0; w < 3 && !e; w++)
    e = yhk_wide_collapse(2 + w, T.num_nodes, (const float*)T.d_tree.p, (const unsigned int*)T.d_wflag[w].p, (const unsigned int*)T.d_widx[w].p,
        L.kind == YH_KIND_LINES ? 1 : 0, offs[w], L.test_off, blob, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%swide collapse: %s", who, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

// What a built shape leaves for its edits (context_internal.h: ShapeState): depths, counts, the room of its regions of the traversal array
// (the upload: exactly its nodes; yh_update_shape: what it chose, blob_layout.h), the levels of its wide trees, and the slot areas as built.
void shape_state_of_build(yh_context::ShapeState& E, const ShapeTree& T, const int room[3], const double area[3]) {
  E.depth = T.depth, E.depth8 = T.depth8, E.depth16 = T.depth16;
  for (int w = 0; w < 3; w++) {
    E.count[w] = T.wide_count[w], E.room[w] = room[w];
    E.wide_levels[w] = T.wide_levels[w];
    memcpy(E.wide_first[w], T.wide_first[w], sizeof(E.wide_first[w]));
    E.area_build[w] = E.area_now[w] = area[w];
  }
}

// ---- yh_upload_scene_maps, a stage at a time. The stages hand each other one UploadStage; what can refuse after drop_previous_scene leaves a
// context WITHOUT a scene (every launch then says "before yh_upload_scene"), never one whose scene table points at freed arrays. ----------------
namespace {
struct UploadShape : ShapeTree {
  int prim_base, vert_base, elem_base, has_normals;
};
struct UploadStage {
  const yh_scene_desc*      sd   = nullptr;
  const yh_material_maps*   maps = nullptr;  // the caller's, where some material has an effective map; else NULL
  std::vector<UploadShape>  shapes;
  size_t                    total_prim_f4 = 0;
  std::vector<yhd_float4>   vpos;   // the per-vertex rows of the shapes that have some (upload_shapes)
  std::vector<float>        vtex;   // 2 per vertex, zeros for shapes without texture coordinates
  std::vector<yhd_int4>     elems;
  std::vector<yhh::Box>     obj_boxes, shape_roots;
  SceneLevelStage           level;
  BlobLayout                blob;
  std::vector<double>       slot_areas;  // 3 per shape
  std::vector<yhd_object>   objects;
  std::vector<yhd_material> materials;
  std::vector<yhd_maps>     mat_maps;
  bool                      general_rows = false;
  yhd_scene                 sc{};  // the scene table: the environments' rows and the lights from upload_lights on, the rest at fill_scene_table
  LightLayout               lights;
  std::vector<yhd_float4>   env_texels, light_table, tex_texels;
  std::vector<float>        light_cdf, env_tab;
  std::vector<yhd_texture>  textures;
};
}  // namespace

// The checks that run before anything of the context is freed: a refusal here leaves the previous scene in place.
static int check_upload(yh_context* ctx, const yh_scene_desc* sd, const yh_material_maps* maps, UploadStage& U) {
  if (!sd) return fail(ctx, YH_E_INVALID, "scene is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->poisoned) return refuse_poisoned(ctx);
  YH_WAIT(ctx);  // (an asynchronous launch may still be reading the scene this call replaces: wait for it, within the deadline)
  if (sd->num_objects <= 0) return fail(ctx, YH_E_INVALID, "scene has no objects");
  if (sd->num_environments > YH_MAX_ENVS) return fail(ctx, YH_E_INVALID, "more than %d environments", YH_MAX_ENVS);
  bool any_maps = false;
  if (maps)
    for (int i = 0; i < sd->num_materials; i++) {
      const yh_material_maps& m = maps[i];
      for (int id : {m.specular_tex, m.metallic_tex, m.roughness_tex, m.transmission_tex, m.opacity_tex, m.normal_tex})
        if (id < 0 || id > sd->num_textures) return fail(ctx, YH_E_INVALID, "material %d: a map references a missing texture (%d of %d)", i, id, sd->num_textures);
      any_maps = any_maps || has_effective_map(m);
    }
  U.sd = sd, U.maps = any_maps ? maps : nullptr;
  U.shapes.resize((size_t)sd->num_shapes);
  for (int si = 0; si < sd->num_shapes; si++) {
    auto& s = sd->shapes[si];
    auto& I = U.shapes[(size_t)si];
    if (s.num_vertices <= 0 || !s.positions) return fail(ctx, YH_E_INVALID, "shape %d has no vertices", si);
    const bool lines = s.num_lines > 0;
    if (!lines && s.num_triangles <= 0) return fail(ctx, YH_E_INVALID, "shape %d has no lines or triangles", si);
    const int nel = lines ? s.num_lines : s.num_triangles;
    // a leaf reference packs its first record into 27 bits (host/bvh_build.cpp: count << 27 | start)
    if (nel >= (1 << 27)) return fail(ctx, YH_E_INVALID, "shape %d has %d elements (limit %d)", si, nel, (1 << 27) - 1);
    I.kind = lines ? YH_KIND_LINES : YH_KIND_TRIANGLES, I.num_prims = nel, I.has_normals = s.normals != nullptr;
    I.prim_base = (int)U.total_prim_f4;
    U.total_prim_f4 += (size_t)nel * (lines ? 4 : 6);
  }
  if (U.total_prim_f4 > (size_t)std::numeric_limits<int>::max())
    return fail(ctx, YH_E_INVALID, "scene too large for 32-bit record offsets (%zu primitive float4)", U.total_prim_f4);
  return YH_OK;
}

// The one place that drops the previous scene: from here on its device arrays are being replaced.
static void drop_previous_scene(yh_context* ctx) {
  ctx->have_scene = false, ctx->have_state = false;
  temporal_drop(ctx);  // (another scene's history)
  ctx->scene.lane_blob = nullptr, ctx->scene.prims = nullptr;
  ctx->d_prims.reset(), ctx->d_lane_blob.reset();  // (nothing of this context is running: waited for above)
  for (DevBuf& kept : ctx->d_env_cdf) kept.reset();  // (the texel cdfs a light edit kept: another scene's)
}

// Per shape: the index check, the tree with its leaf-ordered records (build_shape_tree above: big shapes on the device, small ones on the
// host), and its rows of the per-vertex arrays.
static int upload_shapes(yh_context* ctx, UploadStage& U, Lap& lap) {
  const yh_scene_desc* sd = U.sd;
  for (int si = 0; si < sd->num_shapes; si++) {
    auto&      s     = sd->shapes[si];
    auto&      I     = U.shapes[(size_t)si];
    const bool lines = I.kind == YH_KIND_LINES;
    const int  nel   = I.num_prims;
    const int* idx   = lines ? s.lines : s.triangles;
    {  // (a parallel pass: 3.2 M indices of a hair model)
      std::atomic<bool> bad{false};
      parallel_for(nel * (lines ? 2 : 3), [&](int k) {
        if (idx[k] < 0 || idx[k] >= s.num_vertices) bad = true;
      });
      if (bad) return fail(ctx, YH_E_INVALID, "shape %d: vertex index out of range", si);
    }
    if (int rc = build_shape_tree(ctx, "", si, s, false, shape_builds_on_device(nel), (yhd_float4*)ctx->d_prims.p + I.prim_base, I)) return rc;
    lap(I.host_prims.empty() ? "device: bounds, tree, leaf records" : "host: small shape");
    // Per-vertex positions and per-element indices are read on the device only to sample a point
    // on an area light (triangles, pt.cpp:1287-1292) and to interpolate texture coordinates; the
    // traversal and the shading of a hit use the leaf records. Hair without texture coordinates —
    // nearly all of a scene's bytes — therefore has no entry in these arrays.
    I.vert_base = 0, I.elem_base = 0;
    if (lines && !s.texcoords) continue;
    const size_t at = U.vpos.size(), ea = U.elems.size();
    I.vert_base = (int)at, I.elem_base = (int)ea;
    U.vpos.resize(at + (size_t)s.num_vertices);
    U.vtex.resize(2 * (at + (size_t)s.num_vertices), 0.0f);
    if (s.texcoords) memcpy(&U.vtex[2 * at], s.texcoords, sizeof(float) * 2 * (size_t)s.num_vertices);
    parallel_for(s.num_vertices, [&](int v) {
      F3 p = ld3(s.positions + 3 * (size_t)v);
      U.vpos[at + (size_t)v] = {p.x, p.y, p.z, lines ? (s.radius ? s.radius[v] : 0.001f) : 0.0f};
    });
    U.elems.resize(ea + (size_t)nel);
    parallel_for(nel, [&](int e) {
      U.elems[ea + (size_t)e] = lines ? yhd_int4{idx[2 * e], idx[2 * e + 1], 0, 0} : yhd_int4{idx[3 * e], idx[3 * e + 1], idx[3 * e + 2], 0};
    });
  }
  return YH_OK;
}

// The scene level (pt.cpp:792-814): the objects' world boxes and what follows from the reference's tree over them (derive_scene_level).
static int upload_scene_level(yh_context* ctx, UploadStage& U) {
  const yh_scene_desc* sd = U.sd;
  U.obj_boxes.resize((size_t)sd->num_objects);
  for (int oi = 0; oi < sd->num_objects; oi++) {
    auto& o = sd->objects[oi];
    if (o.shape < 0 || o.shape >= sd->num_shapes || o.material < 0 || o.material >= sd->num_materials)
      return fail(ctx, YH_E_INVALID, "object %d references a missing shape or material", oi);
    const yhh::Box& b = U.shapes[(size_t)o.shape].root;
    transform_bbox(o.frame, b.min, b.max, U.obj_boxes[(size_t)oi].min, U.obj_boxes[(size_t)oi].max);  // (unit/object_math.h)
  }
  const ShapeDepths deepest = deepest_shape_trees(U.shapes);
  return derive_scene_level(ctx, "", U.obj_boxes, sd->num_objects, deepest.depth4, deepest.depth8, deepest.depth16, U.level);
}

// The ONE array the traversal kernels read: the index of every wide node (one flag pass + one scan per width), where everything sits
// (blob_layout.h), the allocation, the collapses, and the half-area sums of every shape's slot boxes as built (what yh_shape_refit_growth
// compares a refitted tree with). The binary trees go when it is made.
static int upload_traversal_array(yh_context* ctx, UploadStage& U) {
  const int num_shapes = (int)U.shapes.size();
  for (auto& I : U.shapes)
    if (int rc = index_shape_tree(ctx, "", I)) return rc;
  std::vector<BlobShape> in;
  for (auto& I : U.shapes) in.push_back({I.kind == YH_KIND_LINES, I.num_prims, {I.wide_count[0], I.wide_count[1], I.wide_count[2]}});
  long long at = 0;
  switch (blob_layout(U.level.scene_wide, U.sd->num_objects, in.data(), num_shapes, U.blob, &at)) {
    case YH_BLOB_LEAF_OFFSETS: return fail(ctx, YH_E_INVALID, "scene too large for 27-bit leaf offsets (%lld test-record units)", at);
    case YH_BLOB_NODE_OFFSETS: return fail(ctx, YH_E_INVALID, "scene too large for 30-bit node offsets (%lld units)", at);
  }
  ctx->lane_shapes.assign((size_t)num_shapes, yh_context::LaneShape{});
  for (int si = 0; si < num_shapes; si++) {
    const auto& I = U.shapes[(size_t)si];
    const auto& R = U.blob.shapes[(size_t)si];
    ctx->lane_shapes[(size_t)si] = {I.kind, I.wide_count[0], I.prim_base, I.num_prims, R.node_off[0], R.test_off, R.node_off[1], R.node_off[2]};
  }
  ctx->lane_units = U.blob.lane_units;
  if (int rc = alloc_zero(ctx, ctx->d_lane_blob, (size_t)U.blob.units * 32)) return rc;
  for (int si = 0; si < num_shapes; si++)
    if (int rc = collapse_shape_tree(ctx, "", U.shapes[(size_t)si], ctx->lane_shapes[(size_t)si], ctx->d_lane_blob.p)) return rc;
  if (int rc = collapse_scene_tree(ctx, U.level, ctx->d_lane_blob.p)) return rc;
  U.slot_areas.resize(3 * (size_t)num_shapes);
  {
    std::vector<int> counts(3 * (size_t)num_shapes);
    for (int si = 0; si < num_shapes; si++) memcpy(&counts[3 * (size_t)si], U.shapes[(size_t)si].wide_count, sizeof(U.shapes[(size_t)si].wide_count));
    if (int rc = shape_slot_areas(ctx, "", num_shapes, ctx->lane_shapes.data(), (const int(*)[3])counts.data(), ctx->d_lane_blob.p, U.slot_areas.data())) return rc;
  }
  YH_WAIT(ctx);
  for (auto& I : U.shapes) {
    I.d_tree.reset();
    for (int w = 0; w < 3; w++) I.d_wflag[w].reset(), I.d_widx[w].reset();
  }
  U.level.d_stree.reset(), U.level.d_sflag.reset(), U.level.d_sidx.reset();
  return YH_OK;
}

// The object rows (upload_stages.h: object_row), and the two limits the device's offsets and stacks set.
static int upload_object_rows(yh_context* ctx, UploadStage& U) {
  const yh_scene_desc* sd = U.sd;
  U.objects.resize((size_t)sd->num_objects);
  for (int oi = 0; oi < sd->num_objects; oi++) {
    const yh_object& o = sd->objects[oi];
    const auto&      I = U.shapes[(size_t)o.shape];
    const auto&      R = U.blob.shapes[(size_t)o.shape];
    object_row(o, {I.kind, I.prim_base, I.vert_base, I.elem_base, I.has_normals, sd->shapes[o.shape].texcoords != nullptr, R.test_off, {R.node_off[0], R.node_off[1], R.node_off[2]}},
        U.obj_boxes[(size_t)oi], U.objects[(size_t)oi]);
  }
  // array offsets on the device are 32-bit float4 indices
  if (U.vpos.size() > (size_t)std::numeric_limits<int>::max()) return fail(ctx, YH_E_INVALID, "scene too large for 32-bit vertex offsets (%zu)", U.vpos.size());
  return check_stack_needs(ctx, "", U.level.needs);
}

// Materials, environments and the lights (pt.cpp:1695-1740): which they are and where their entries sit is light_layout.h's rule; the cdf
// values, the small lights' records and the index entries are upload_stages.h's, from the arrays the caller lent.
static int upload_lights(yh_context* ctx, UploadStage& U) {
  const yh_scene_desc* sd = U.sd;
  U.materials.resize((size_t)sd->num_materials);
  U.mat_maps.resize(U.maps ? (size_t)sd->num_materials : 0);
  U.general_rows = make_material_rows(sd->materials, U.maps, sd->num_materials, U.materials.data(), U.mat_maps.data());
  U.sc.num_environments = sd->num_environments;
  float env_emission[3 * YH_MAX_ENVS] = {};
  int   env_texel_count[YH_MAX_ENVS]  = {};
  environment_rows(*sd, U.sc.environments, U.env_texels, env_emission, env_texel_count);
  std::vector<LightShape> light_shapes;
  for (auto& I : U.shapes) light_shapes.push_back({I.kind == YH_KIND_LINES, I.num_prims});
  int at = 0;
  switch (light_layout({sd->num_objects, sd->objects, sd->materials, light_shapes.data(), sd->num_environments, env_emission, env_texel_count}, U.lights, &at)) {
    // (every object with an emissive material is a light of its own, so every frame of an instanced emitter is one: init_lights walks objects)
    case YH_LIGHTS_OBJECT_TOO_MANY:
      return fail(ctx, YH_E_INVALID, "more than %d lights: object %d of %d is emissive too (each instance of an emitter counts)", YH_MAX_LIGHTS, at, sd->num_objects);
    case YH_LIGHTS_ENVIRONMENT_TOO_MANY: return fail(ctx, YH_E_INVALID, "more than %d lights", YH_MAX_LIGHTS);
    case YH_LIGHTS_NONE: return fail(ctx, YH_E_INVALID, "scene has no lights (the path sampler needs at least one)");
  }
  light_cdfs(*sd, U.lights, U.light_cdf);
  for (int li = 0; li < U.lights.num_lights; li++) {
    const yhd_light& L = U.lights.lights[li];
    if (L.small_base < 0) continue;  // (light_table.size() is L.small_base here: the records follow each other in list order)
    auto& I = U.shapes[(size_t)sd->objects[L.object].shape];
    if (I.host_prims.empty()) {  // (a shape made on the device — YHAIR_BVH=device: a light of <= 4 triangles is otherwise a small shape): its few records back
      I.host_prims.resize((size_t)6 * L.cdf_count);
      HIPCHK(ctx, hipMemcpy(I.host_prims.data(), (const yhd_float4*)ctx->d_prims.p + I.prim_base, I.host_prims.size() * 16, hipMemcpyDeviceToHost));
    }
    small_light_record(L, I.root, I.host_prims.data(), U.light_cdf.data(), U.light_table);
  }
  coarse_index(U.lights, U.light_cdf.data(), U.env_tab);
  return YH_OK;
}

static int upload_textures(yh_context* ctx, UploadStage& U) {
  int at = 0;
  switch (convert_textures(*U.sd, U.maps, U.textures, U.tex_texels, &at)) {
    case YH_TEXTURES_MISSING: return fail(ctx, YH_E_INVALID, "material %d references a missing texture", at);
    case YH_TEXTURES_EMPTY: return fail(ctx, YH_E_INVALID, "texture %d is empty", at);
  }
  return YH_OK;
}

// The copies to the device ...
static int upload_arrays(yh_context* ctx, UploadStage& U) {
  int rc;
  if ((rc = upload(ctx, ctx->d_vpos, U.vpos.data(), U.vpos.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_elems, U.elems.data(), U.elems.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_objects, U.objects.data(), U.objects.size() * sizeof(yhd_object)))) return rc;
  if ((rc = upload(ctx, ctx->d_materials, U.materials.data(), U.materials.size() * sizeof(yhd_material)))) return rc;
  if ((rc = upload(ctx, ctx->d_scene_nodes, U.level.scene_nodes.data(), U.level.scene_nodes.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_scene_prims, U.level.scene_prims.data(), U.level.scene_prims.size() * 4))) return rc;
  if ((rc = upload(ctx, ctx->d_light_cdf, U.light_cdf.data(), U.light_cdf.size() * 4))) return rc;
  if ((rc = upload(ctx, ctx->d_light_table, U.light_table.data(), U.light_table.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_env_tab, U.env_tab.data(), U.env_tab.size() * 4))) return rc;
  if ((rc = upload(ctx, ctx->d_env_texels, U.env_texels.data(), U.env_texels.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_textures, U.textures.data(), U.textures.size() * sizeof(yhd_texture)))) return rc;
  if ((rc = upload(ctx, ctx->d_tex_texels, U.tex_texels.data(), U.tex_texels.size() * 16))) return rc;
  if ((rc = upload(ctx, ctx->d_vtex, U.vtex.data(), U.vtex.size() * 4))) return rc;
  for (auto& I : U.shapes) U.shape_roots.push_back(I.root);  // (what yh_update_objects starts from: context_internal.h)
  if ((rc = upload(ctx, ctx->d_shape_roots, U.shape_roots.data(), U.shape_roots.size() * sizeof(yhh::Box)))) return rc;
  if (U.maps) return upload(ctx, ctx->d_maps, U.mat_maps.data(), U.mat_maps.size() * sizeof(yhd_maps));
  ctx->d_maps.reset();
  return YH_OK;
}

// ... and the scene table over them
static void fill_scene_table(yh_context* ctx, UploadStage& U) {
  const yh_scene_desc* sd = U.sd;
  yhd_scene&           sc = U.sc;
  sc.prims = (const yhd_float4*)ctx->d_prims.p;
  sc.vpos = (const yhd_float4*)ctx->d_vpos.p;
  sc.elems = (const yhd_int4*)ctx->d_elems.p;
  sc.objects = (const yhd_object*)ctx->d_objects.p, sc.materials = (const yhd_material*)ctx->d_materials.p;
  sc.num_objects = sd->num_objects;
  sc.env_texels = (const yhd_float4*)ctx->d_env_texels.p;
  sc.lane_blob = (const yhd_float4*)ctx->d_lane_blob.p, sc.lane_blob_units = U.blob.units;
  sc.textures = (const yhd_texture*)ctx->d_textures.p, sc.tex_texels = (const yhd_float4*)ctx->d_tex_texels.p;
  sc.vtex = (const float*)ctx->d_vtex.p;
  sc.maps = U.maps ? (const yhd_maps*)ctx->d_maps.p : nullptr;
  memcpy(sc.camera.frame, sd->camera.frame, 48);
  sc.camera.lens = sd->camera.lens, sc.camera.film_x = sd->camera.film[0], sc.camera.film_y = sd->camera.film[1];
  sc.camera.focus = sd->camera.focus, sc.camera.aperture = sd->camera.aperture;
  sc.num_nodes_total = 0, sc.num_prim_f4 = (int)U.total_prim_f4;
  for (auto& I : U.shapes) sc.num_nodes_total += I.wide_count[0];
  static_assert(sizeof(yhd_material) == 16 * YH_MATERIAL_F4, "yhd_material is staged to LDS as float4");
  sc.lds_materials = sd->num_materials <= 24 ? sd->num_materials : 0;  // the material table in LDS
  set_scene_level_fields(ctx, sc, U.level);
  set_light_fields(ctx, sc, U.lights);
  settle_scene_variant(ctx, sc, U.general_rows);
  ctx->scene = sc;
}

// What the edits of this scene start from (host/edit_internal.h), and its fingerprint over the bytes the context keeps of the description.
static void keep_for_edits(yh_context* ctx, UploadStage& U) {
  const yh_scene_desc* sd = U.sd;
  ctx->key_camera = sd->camera;
  ctx->h_materials.assign(sd->materials, sd->materials + sd->num_materials);
  std::vector<size_t> key_positions;
  description_key_bytes(*sd, ctx->key_geometry, ctx->key_envs, key_positions);
  ctx->shape_states.assign((size_t)sd->num_shapes, yh_context::ShapeState{});
  for (int i = 0; i < sd->num_shapes; i++) {  // (at an upload every width has room for exactly its nodes)
    const yh_shape& sh = sd->shapes[i];
    auto&           E  = ctx->shape_states[(size_t)i];
    const auto&     I  = U.shapes[(size_t)i];
    E.num_vertices = sh.num_vertices, E.has_normals = sh.normals != nullptr, E.has_texcoords = sh.texcoords != nullptr;
    E.per_vertex = sh.num_lines <= 0 || sh.texcoords != nullptr, E.vert_base = I.vert_base, E.elem_base = I.elem_base;
    E.key_positions = key_positions[(size_t)i];
    shape_state_of_build(E, I, I.wide_count, &U.slot_areas[3 * (size_t)i]);
  }
  if (U.maps) ctx->h_maps.assign(U.maps, U.maps + sd->num_materials), ctx->h_dmaps = U.mat_maps;
  else ctx->h_maps.clear(), ctx->h_dmaps.clear();
  ctx->h_shape_roots.swap(U.shape_roots), ctx->h_obj_boxes.swap(U.obj_boxes);
  const ShapeDepths deepest = deepest_shape_trees(U.shapes);
  ctx->max_shape_depth = deepest.depth4, ctx->max_shape_depth8 = deepest.depth8, ctx->max_shape_depth16 = deepest.depth16;
  ctx->scene_wide_room = U.level.scene_wide ? sd->num_objects : 0;
  ctx->scene_key = scene_fingerprint(ctx);
}

int yh_upload_scene(yh_context* ctx, const yh_scene_desc* sd) { return yh_upload_scene_maps(ctx, sd, nullptr); }

int yh_upload_scene_maps(yh_context* ctx, const yh_scene_desc* sd, const yh_material_maps* maps) {
  if (!ctx) return YH_E_INVALID;
  Lap         lap("upload");  // YHAIR_TIMING=1: stage times of the upload on stderr
  UploadStage U;
  if (int rc = check_upload(ctx, sd, maps, U)) return rc;
  drop_previous_scene(ctx);
  if (int rc = dev_alloc(ctx, ctx->d_prims, U.total_prim_f4 * 16)) return rc;
  lap("validation, record array");
  if (int rc = upload_shapes(ctx, U, lap)) return rc;
  if (int rc = upload_scene_level(ctx, U)) return rc;
  if (int rc = upload_traversal_array(ctx, U)) return rc;
  lap("device: wide collapses, blob");
  if (int rc = upload_object_rows(ctx, U)) return rc;
  if (int rc = upload_lights(ctx, U)) return rc;
  if (int rc = upload_textures(ctx, U)) return rc;
  lap("objects, materials, lights");
  if (int rc = upload_arrays(ctx, U)) return rc;
  lap("hipMalloc + H2D copies");
  fill_scene_table(ctx, U);
  keep_for_edits(ctx, U);
  ctx->have_scene = true;
  forget_image_of_scene(ctx);  // a new scene: no measured costs yet
  lap("scene table, fingerprint");
  return YH_OK;
}

// The same tree built on the device (csrc/bvh_gpu.hip): fills `tree` like yhh::build_bvh.
int build_bvh_device(yh_context* ctx, const std::vector<yhh::Box>& boxes, yhh::Tree& tree) {
  int                n = (int)boxes.size(), num_nodes = 0, depth = 0;
  std::vector<float> nodes8((size_t)(2 * n + 1) * 8);
  tree.primitives.resize((size_t)n);
  static_assert(sizeof(yhh::Box) == 24, "boxes are passed as 6 floats");
  int e = yhk_bvh_build_gpu(n, (const float*)boxes.data(), nodes8.data(), tree.primitives.data(), &num_nodes, &depth, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "device BVH build: %s", hipGetErrorString((hipError_t)e));
  tree.nodes.resize((size_t)num_nodes);
  tree.max_depth = depth;
  for (int i = 0; i < num_nodes; i++) {
    const float* o  = &nodes8[(size_t)i * 8];
    yhh::Node&   nd = tree.nodes[(size_t)i];
    memcpy(nd.bbox.min, o, 12), memcpy(nd.bbox.max, o + 3, 12);
    int start, meta;
    memcpy(&start, o + 6, 4), memcpy(&meta, o + 7, 4);
    nd.start = start, nd.num = (short)(meta & 0xFFFF), nd.internal = (meta >> 16) & 1, nd.axis = (unsigned char)((meta >> 24) & 3);
  }
  return YH_OK;
}
