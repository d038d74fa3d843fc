// scene_edit.cpp — edits of an uploaded scene: the camera, rows of the material table, the environments' frames and emission, rows of the
// object list (yh_update_objects: it builds the scene-level tree over the objects' world boxes again) and, at the end, one shape's vertices
// (yh_update_shape / _device: that shape's tree, records and nodes again, then the scene level; no other shape is touched; yh_refit_shape /
// _device: the same edit in the tree the shape has, its records and boxes only). The reference
// reads its scene structs live (an interactive caller edits app->camera->frame and traces on,
// apps/ysceneitraces/ysceneitraces.cpp:392-410); here the description was flattened at yh_upload_scene, so an edit is a call of its own
// that leaves the context as an upload of the edited description would: the scene table, the material rows on the device, the kernel
// variant, the once-per-ray form, the fingerprint and the launch planning. Only a shape edit reads, writes or allocates anything the geometry sizes, and then the edited shape's alone.
// yh_set_light_edits (off by default): the seven edits that would change the light list make it again by the upload's rule instead of
// refusing (stage_lights / commit_lights below, unit/light_list.hip): the area cdfs, the small lights' records and the coarse index of a
// texel cdf on the device, from the rows the context keeps there.
// Also yh_download_display, the tone-mapped bytes of the image (unit/display.hip).
#include "context_internal.h"

static bool is_black(const float* e) { return e[0] == 0 && e[1] == 0 && e[2] == 0; }

// what every edit starts with: a context that can take it
static int edit_begin(yh_context* ctx, const char* entry) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->poisoned) return fail(ctx, YH_E_DEVICE, "a launch of this context exceeded its deadline: the context refuses further work, destroy it");
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "%s before yh_upload_scene", entry);
  YH_WAIT(ctx);  // (an asynchronous launch may still be reading the tables this call rewrites: wait for it, within the deadline)
  return YH_OK;
}
// ... and ends with: the image state is gone and the next yh_init_state probes and plans as for a new scene
static void edit_end(yh_context* ctx) {
  ctx->scene_key = scene_fingerprint(ctx);
  forget_image_of_scene(ctx);
}

// a device allocation of an edit's staging
static int stage_alloc(yh_context* ctx, DevBuf& buf, size_t bytes) {
  buf.reset();
  HIPCHK(ctx, hipMalloc(&buf.p, std::max<size_t>(bytes, 16)));
  buf.bytes = std::max<size_t>(bytes, 16);
  return YH_OK;
}

// ---- the light list again (yh_set_light_edits): init_lights' rule as the upload runs it (scene_upload.cpp), over the description the context
// keeps and the edit at hand. stage_lights walks the objects and the environments in order, refuses what the upload refuses (more than
// YH_MAX_LIGHTS lights, none at all), lays out the new light_cdf and light table, allocates them and sees to it that every textured
// environment of the new list has its texel cdf on the device (ctx->d_env_cdf: saved from the light_cdf in force, or made with the
// upload's loop from the texels read back from d_env_texels — the host's sine, scene_upload.cpp: append_env_cdf). Nothing the kernels
// read is written. commit_lights queues the kernels and copies into the NEW arrays on the context's stream and brings the scene table
// in line; the old arrays go when the stage does, after the caller's wait. (A vertex edit of an emitter's shape moves no light:
// stage_lights_of_shape / commit_lights_of_shape below write the entries of that shape's lights where they are.) ----
namespace {
struct LightStage {
  int       num_lights = 0;
  yhd_light lights[YH_MAX_LIGHTS] = {};
  bool      big_lights = false;
  int       table_f4 = 0, env_tab_light = -1, env_tab_k = 0, env_tab_stride = 0;
  size_t    cdf_total = 0;
  std::vector<yhk_light_job> jobs;  // the area lights, in list order
  DevBuf    d_jobs, d_cdf, d_table, d_tab;
};
}  // namespace

// materials: the whole table as the edit leaves it; rows: every object row; emission: 3 floats per environment
static int stage_lights(yh_context* ctx, const char* entry, const yh_material* materials, const yh_object* rows, const float* emission, LightStage& S) {
  const yhd_scene& sc = ctx->scene;
  for (int oi = 0; oi < sc.num_objects; oi++) {
    const yh_object& o = rows[oi];
    if (is_black(materials[o.material].emission)) continue;
    const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)o.shape];
    const yh_context::ShapeState& E = ctx->shape_states[(size_t)o.shape];
    if (L.kind == YH_KIND_LINES || L.num_prims <= 0) continue;  // a line shape never becomes a light
    if (S.num_lights >= YH_MAX_LIGHTS)
      return fail(ctx, YH_E_INVALID, "%s: more than %d lights: object %d of %d is emissive too (each instance of an emitter counts)", entry, YH_MAX_LIGHTS, oi, sc.num_objects);
    yhd_light& l = S.lights[S.num_lights++];
    l.object = oi, l.environment = -1, l.cdf_base = (int)S.cdf_total, l.cdf_count = L.num_prims, l.small_base = -1;
    if (L.num_prims <= YH_SMALL_LIGHT_TRIS) l.small_base = S.table_f4, S.table_f4 += YH_SMALL_LIGHT_F4;
    else S.big_lights = true;
    S.jobs.push_back({E.elem_base, E.vert_base, L.num_prims, l.cdf_base, L.prim_base, o.shape, l.small_base, 0});
    S.cdf_total += (size_t)L.num_prims;
  }
  for (int ei = 0; ei < sc.num_environments; ei++) {
    if (is_black(emission + 3 * ei)) continue;
    if (S.num_lights >= YH_MAX_LIGHTS) return fail(ctx, YH_E_INVALID, "%s: more than %d lights: environment %d is one too", entry, YH_MAX_LIGHTS, ei);
    yhd_light& l = S.lights[S.num_lights++];
    l.object = -1, l.environment = ei, l.cdf_base = (int)S.cdf_total, l.small_base = -1;
    l.cdf_count = sc.environments[ei].tex_w * sc.environments[ei].tex_h;  // (0 x 0 for a constant one: no cdf)
    S.cdf_total += (size_t)l.cdf_count;
  }
  if (S.num_lights == 0) return fail(ctx, YH_E_INVALID, "%s: the edit leaves the scene without a light (the path sampler needs at least one): upload the scene", entry);
  if (S.cdf_total > (size_t)std::numeric_limits<int>::max()) return fail(ctx, YH_E_INVALID, "%s: light cdf of %zu entries", entry, S.cdf_total);
  for (int li = 0; li < S.num_lights && S.env_tab_light < 0; li++) {  // the first textured environment light of at least 4096 texels
    const yhd_light& l = S.lights[li];
    if (l.environment < 0 || l.cdf_count < 4096) continue;
    const int n = l.cdf_count, stride = (n + 2047) / 2048;
    S.env_tab_light = li, S.env_tab_k = (n + stride - 1) / stride, S.env_tab_stride = stride;
  }
  // the texel cdf of every textured environment that is a light now or will be one: kept on the device from here on. (A cache that no
  // entry point shows and whose content depends on the texels alone: a call refused further down leaves it filled, and is still
  // "the context exactly as it was" for everything a caller can observe.)
  auto kept = [&](int ei, int count, const float* d_segment) -> int {
    DevBuf& buf = ctx->d_env_cdf[ei];
    if (buf.p || count <= 0) return YH_OK;
    DevBuf made;
    if (int rc = stage_alloc(ctx, made, (size_t)count * 4)) return rc;
    if (d_segment) {
      HIPCHK(ctx, hipMemcpyAsync(made.p, d_segment, (size_t)count * 4, hipMemcpyDeviceToDevice, ctx->stream));  // (commit_lights copies from it on the same stream)
    } else {  // its first turn as a light: the upload's loop over the floats the upload was given
      const yhd_environment& e = sc.environments[ei];
      std::vector<yhd_float4> texels((size_t)count);
      std::vector<float>      cdf;
      HIPCHK(ctx, hipMemcpy(texels.data(), (const yhd_float4*)ctx->d_env_texels.p + e.texel_base, texels.size() * 16, hipMemcpyDeviceToHost));
      cdf.reserve(texels.size());
      append_env_cdf(&texels[0].x, 4, e.tex_w, e.tex_h, cdf);
      HIPCHK(ctx, hipMemcpy(made.p, cdf.data(), cdf.size() * 4, hipMemcpyHostToDevice));
    }
    std::swap(buf.p, made.p), std::swap(buf.bytes, made.bytes);
    return YH_OK;
  };
  for (int li = 0; li < sc.num_lights; li++)
    if (sc.lights[li].environment >= 0)
      if (int rc = kept(sc.lights[li].environment, sc.lights[li].cdf_count, (const float*)ctx->d_light_cdf.p + sc.lights[li].cdf_base)) return rc;
  for (int li = 0; li < S.num_lights; li++)
    if (S.lights[li].environment >= 0)
      if (int rc = kept(S.lights[li].environment, S.lights[li].cdf_count, nullptr)) return rc;
  if (int rc = stage_alloc(ctx, S.d_cdf, S.cdf_total * 4)) return rc;
  if (int rc = stage_alloc(ctx, S.d_table, (size_t)S.table_f4 * 16)) return rc;
  if (int rc = stage_alloc(ctx, S.d_tab, (size_t)S.env_tab_k * 4)) return rc;
  if (int rc = stage_alloc(ctx, S.d_jobs, S.jobs.size() * sizeof(yhk_light_job))) return rc;
  return YH_OK;
}

static int commit_lights(yh_context* ctx, const char* entry, LightStage& S) {
  const int nj = (int)S.jobs.size();
  if (nj > 0) HIPCHK(ctx, hipMemcpyAsync(S.d_jobs.p, S.jobs.data(), S.jobs.size() * sizeof(yhk_light_job), hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_light_cdfs(nj, S.d_jobs.p, ctx->d_vpos.p, ctx->d_elems.p, (float*)S.d_cdf.p, ctx->stream);
  if (!e) e = yhk_small_records(nj, S.d_jobs.p, (const float*)ctx->d_shape_roots.p, ctx->d_prims.p, (const float*)S.d_cdf.p, S.d_table.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: light list: %s", entry, hipGetErrorString((hipError_t)e));
  for (int li = 0; li < S.num_lights; li++) {  // an environment light's segment: a copy of the cdf the context keeps
    const yhd_light& l = S.lights[li];
    if (l.environment >= 0 && l.cdf_count > 0)
      HIPCHK(ctx, hipMemcpyAsync((float*)S.d_cdf.p + l.cdf_base, ctx->d_env_cdf[l.environment].p, (size_t)l.cdf_count * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  if (S.env_tab_light >= 0) {
    const yhd_light& l = S.lights[S.env_tab_light];
    e = yhk_env_tab(S.env_tab_k, S.env_tab_stride, l.cdf_count, (const float*)S.d_cdf.p + l.cdf_base, (float*)S.d_tab.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%s: coarse index of the environment cdf: %s", entry, hipGetErrorString((hipError_t)e));
  }
  auto take = [](DevBuf& mine, DevBuf& staged) { std::swap(mine.p, staged.p), std::swap(mine.bytes, staged.bytes); };
  take(ctx->d_light_cdf, S.d_cdf), take(ctx->d_light_table, S.d_table), take(ctx->d_env_tab, S.d_tab);
  yhd_scene& sc = ctx->scene;
  sc.num_lights = S.num_lights;
  memcpy(sc.lights, S.lights, sizeof(sc.lights));
  sc.light_cdf = (const float*)ctx->d_light_cdf.p;
  sc.light_table = (const yhd_float4*)ctx->d_light_table.p, sc.light_table_f4 = S.table_f4;
  sc.env_tab = (const float*)ctx->d_env_tab.p;
  sc.env_tab_light = S.env_tab_light, sc.env_tab_k = S.env_tab_k, sc.env_tab_stride = S.env_tab_stride;
  ctx->big_lights = S.big_lights;  // (settle_scene_variant reads it: the caller runs that next)
  return YH_OK;
}

// A VERTEX edit of an emitter's shape changes no light's place: the list, every offset, the kernel variant and every other light's
// entries stay. Only the lights that name `shape` get their cdf segment and their small record again, written where they are, from the
// rows, records and root box the edit has queued on the stream before. rows: every object row.
static int stage_lights_of_shape(yh_context* ctx, int shape, const yh_object* rows, LightStage& S) {
  const yhd_scene& sc = ctx->scene;
  for (int li = 0; li < sc.num_lights; li++) {
    const yhd_light& l = sc.lights[li];
    if (l.object < 0 || rows[l.object].shape != shape) continue;
    const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)shape];
    const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
    S.jobs.push_back({E.elem_base, E.vert_base, l.cdf_count, l.cdf_base, L.prim_base, shape, l.small_base, 0});
  }
  return stage_alloc(ctx, S.d_jobs, S.jobs.size() * sizeof(yhk_light_job));
}
static int commit_lights_of_shape(yh_context* ctx, const char* entry, LightStage& S) {
  const int nj = (int)S.jobs.size();
  if (nj == 0) return YH_OK;
  HIPCHK(ctx, hipMemcpyAsync(S.d_jobs.p, S.jobs.data(), S.jobs.size() * sizeof(yhk_light_job), hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_light_cdfs(nj, S.d_jobs.p, ctx->d_vpos.p, ctx->d_elems.p, (float*)ctx->d_light_cdf.p, ctx->stream);
  if (!e) e = yhk_small_records(nj, S.d_jobs.p, (const float*)ctx->d_shape_roots.p, ctx->d_prims.p, (const float*)ctx->d_light_cdf.p, ctx->d_light_table.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: light list: %s", entry, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

// the material table's verdict, as the upload and yh_update_materials reach it
static bool general_rows_in_force(const yh_context* ctx) {
  const bool                mapped = !ctx->h_maps.empty();
  const int                 n      = (int)ctx->h_materials.size();
  std::vector<yhd_material> rows((size_t)n);
  std::vector<yhd_maps>     dmaps(mapped ? (size_t)n : 0);
  return make_material_rows(ctx->h_materials.data(), mapped ? ctx->h_maps.data() : nullptr, n, rows.data(), dmaps.data());
}
// every object row as it was passed in (key_geometry begins with them), and the environments' emission in force
static std::vector<yh_object> uploaded_rows(const yh_context* ctx) {
  std::vector<yh_object> rows((size_t)ctx->scene.num_objects);
  memcpy(rows.data(), ctx->key_geometry.data(), sizeof(yh_object) * rows.size());
  return rows;
}
static std::vector<float> emission_in_force(const yh_context* ctx) {
  std::vector<float> em(3 * YH_MAX_ENVS, 0.0f);
  for (int i = 0; i < ctx->scene.num_environments; i++) memcpy(&em[3 * (size_t)i], ctx->scene.environments[i].emission, 12);
  return em;
}

int yh_update_camera(yh_context* ctx, const yh_camera* camera) {
  if (!ctx) return YH_E_INVALID;
  if (!camera) return fail(ctx, YH_E_INVALID, "yh_update_camera: camera is NULL");
  if (int rc = edit_begin(ctx, "yh_update_camera")) return rc;
  auto& c = ctx->scene.camera;
  memcpy(c.frame, camera->frame, 48);
  c.lens = camera->lens, c.film_x = camera->film[0], c.film_y = camera->film[1];
  c.focus = camera->focus, c.aperture = camera->aperture;
  ctx->key_camera = *camera;
  edit_end(ctx);
  return YH_OK;
}

int yh_update_materials(yh_context* ctx, int first, int count, const yh_material* materials) {
  if (!ctx) return YH_E_INVALID;
  if (!materials) return fail(ctx, YH_E_INVALID, "yh_update_materials: materials is NULL");
  if (int rc = edit_begin(ctx, "yh_update_materials")) return rc;
  const int total = (int)ctx->h_materials.size();
  if (first < 0 || count < 0 || first > total || count > total - first)
    return fail(ctx, YH_E_INVALID, "yh_update_materials: rows [%d, %d + %d) are outside the uploaded table of %d materials", first, first, count, total);
  bool lights_change = false;
  for (int i = 0; i < count; i++) {
    const yh_material &was = ctx->h_materials[(size_t)first + i], &now = materials[i];
    // the light list (init_lights, pt.cpp:1695-1740) was made from the shapes' host arrays, which were borrowed for the upload only:
    // with yh_set_light_edits it is made again from the rows the device keeps
    const bool toggles = is_black(was.emission) != is_black(now.emission);
    lights_change = lights_change || toggles;
    if (toggles && !ctx->light_edits)
      return fail(ctx, YH_E_INVALID, "yh_update_materials: material %d turns its emission %s: the light list changes, upload the scene", first + i, is_black(now.emission) ? "off" : "on");
    // which texel copies exist (sRGB-decoded, linear) was decided at the upload
    if (was.emission_tex != now.emission_tex || was.color_tex != now.color_tex || was.scattering_tex != now.scattering_tex)
      return fail(ctx, YH_E_INVALID, "yh_update_materials: material %d names another texture: upload the scene", first + i);
  }
  // the rows, through the upload's own function; the whole table's verdict decides the kernel variant
  const bool                mapped = !ctx->h_maps.empty();
  std::vector<yh_material>  all    = ctx->h_materials;
  std::copy(materials, materials + count, all.begin() + first);
  std::vector<yhd_material> rows((size_t)total);
  std::vector<yhd_maps>     dmaps(mapped ? (size_t)total : 0);
  const bool general_rows = make_material_rows(all.data(), mapped ? ctx->h_maps.data() : nullptr, total, rows.data(), dmaps.data());
  LightStage LS;
  if (lights_change)
    if (int rc = stage_lights(ctx, "yh_update_materials", all.data(), uploaded_rows(ctx).data(), emission_in_force(ctx).data(), LS)) return rc;
  if (lights_change) ctx->have_scene = false;  // (from here on an error leaves the context without a scene)
  if (count > 0)
    HIPCHK(ctx, hipMemcpy((yhd_material*)ctx->d_materials.p + first, rows.data() + first, sizeof(yhd_material) * (size_t)count, hipMemcpyHostToDevice));
  if (mapped && count > 0)  // (a map's record carries the material's opacity before its snap)
    HIPCHK(ctx, hipMemcpy((yhd_maps*)ctx->d_maps.p + first, dmaps.data() + first, sizeof(yhd_maps) * (size_t)count, hipMemcpyHostToDevice));
  if (lights_change) {
    if (int rc = commit_lights(ctx, "yh_update_materials", LS)) return rc;
    YH_WAIT(ctx);
  }
  ctx->h_materials.swap(all);
  if (mapped) ctx->h_dmaps.swap(dmaps);
  settle_scene_variant(ctx, ctx->scene, general_rows);
  ctx->have_scene = true;
  edit_end(ctx);
  return YH_OK;
}

int yh_update_environments(yh_context* ctx, int count, const yh_environment* environments) {
  if (!ctx) return YH_E_INVALID;
  if (!environments && count != 0) return fail(ctx, YH_E_INVALID, "yh_update_environments: environments is NULL");
  if (int rc = edit_begin(ctx, "yh_update_environments")) return rc;
  if (count != ctx->scene.num_environments)
    return fail(ctx, YH_E_INVALID, "yh_update_environments: %d environments, the uploaded scene has %d", count, ctx->scene.num_environments);
  bool lights_change = false;
  for (int i = 0; i < count; i++) {
    const bool toggles = is_black(ctx->scene.environments[i].emission) != is_black(environments[i].emission);
    lights_change = lights_change || toggles;
    if (toggles && !ctx->light_edits)
      return fail(ctx, YH_E_INVALID, "yh_update_environments: environment %d turns its emission %s: the light list changes, upload the scene", i, is_black(environments[i].emission) ? "off" : "on");
  }
  LightStage LS;
  if (lights_change) {
    std::vector<float> em(3 * YH_MAX_ENVS, 0.0f);
    for (int i = 0; i < count; i++) memcpy(&em[3 * (size_t)i], environments[i].emission, 12);
    if (int rc = stage_lights(ctx, "yh_update_environments", ctx->h_materials.data(), uploaded_rows(ctx).data(), em.data(), LS)) return rc;
    ctx->have_scene = false;  // (from here on an error leaves the context without a scene)
    if (int rc = commit_lights(ctx, "yh_update_environments", LS)) return rc;
    YH_WAIT(ctx);
    settle_scene_variant(ctx, ctx->scene, general_rows_in_force(ctx));  // (the index of a texel cdf is one of the kernels' LDS tables)
    ctx->have_scene = true;
  }
  const size_t head = offsetof(yh_environment, texels), edited = offsetof(yh_environment, tex_width);  // frame and emission
  for (int i = 0; i < count; i++) {
    auto& d = ctx->scene.environments[i];
    memcpy(d.frame, environments[i].frame, 48);
    inverse_frame(environments[i].frame, false, d.inv_frame);
    memcpy(d.emission, environments[i].emission, 12);
    memcpy(ctx->key_envs.data() + head * (size_t)i, &environments[i], edited);
  }
  edit_end(ctx);
  return YH_OK;
}

// ---- yh_update_objects: set_frame / set_material on an object (yocto_pathtrace.h:110-111) ------------------------------------------------
// Shape trees live in object space, so a moved object changes its row (frame, inverse, padded world box, material), the reference's scene
// tree over the world boxes and what follows from that tree: the table sizes, the 4-wide scene nodes at the front of the lane blob, the
// stack needs, the kernel variant. The per-object arithmetic runs on the device (unit/objects.hip), the tree is built as the upload
// builds it (yhh::build_bvh on the host, the device's collapse). Everything that can refuse is computed into staging first; from COMMIT
// on only copies, a memset and two kernels run, and an error there leaves the context without a scene, as a failed upload does.
// ---- the scene level again: what yh_update_objects and yh_update_shape share. Everything that can refuse is staged by stage_scene_level;
// commit_scene_level queues the copies, the memset and the collapse on the context's stream; settle_scene_level, once they are done,
// brings the host's side of the scene table in line ----
namespace {
struct SceneLevelStage {
  yhh::Tree  tree;
  int        nn = 0, lds_scene_f4 = 0, wide_count = 0, wide_depth = 0;
  bool       scene_wide = false, general_rows = false;
  DevBuf     d_stree, d_sflag, d_sidx, d_nodes_grown, d_prims_grown;
  StackNeeds needs{};
  std::vector<yhd_float4> scene_nodes;
  std::vector<int>        scene_prims;
};
}  // namespace

// boxes: every object's world box; depth4 / 8 / 16: the deepest shape tree as 4- / 8- / 16-wide nodes
static int stage_scene_level(yh_context* ctx, const char* entry, const std::vector<yhh::Box>& boxes, int depth4, int depth8, int depth16, SceneLevelStage& S) {
  const int total = ctx->scene.num_objects;
  // ---- the scene-level tree, as the upload builds it, and what the upload derives from it ----
  yhh::Tree& tree = S.tree;
  yhh::build_bvh(tree, boxes);
  const int nn = S.nn = (int)tree.nodes.size();
  const bool scene_wide = S.scene_wide = scene_level_is_wide(total, nn, &S.lds_scene_f4), was_wide = ctx->scene.scene_wide_root >= 0;
  if (scene_wide != was_wide)
    return fail(ctx, YH_E_INVALID, "%s: the scene tree of the moved objects has %d nodes and its scene level %s: room for wide scene nodes exists only where the upload put it, upload the scene",
        entry, nn, scene_wide ? "no longer fits the kernels' table (it would be walked as 4-wide nodes)" : "fits the kernels' table again (it was uploaded as 4-wide nodes)");
  if (scene_wide) {
    int levels = 1, level_first[130] = {0};
    if (!tree_levels(tree, levels, level_first)) return fail(ctx, YH_E_INVALID, "%s: scene tree of %d levels", entry, levels);
    if (int rc = stage_alloc(ctx, S.d_stree, (size_t)nn * 32)) return rc;
    if (int rc = stage_alloc(ctx, S.d_sflag, ((size_t)nn + 1) * 4)) return rc;
    if (int rc = stage_alloc(ctx, S.d_sidx, ((size_t)nn + 1) * 4)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(S.d_stree.p, tree.nodes.data(), (size_t)nn * 32, hipMemcpyHostToDevice, ctx->stream));
    int e = yhk_wide_index(nn, (const float*)S.d_stree.p, levels, level_first, 2, (unsigned int*)S.d_sflag.p, (unsigned int*)S.d_sidx.p, &S.wide_count, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "wide-node index of the scene tree: %s", hipGetErrorString((hipError_t)e));
    S.wide_depth = 1 + std::max(0, levels - 2) / 2;
    if (S.wide_count > ctx->scene_wide_room)
      return fail(ctx, YH_E_INVALID, "%s: %d wide scene nodes, the upload left room for %d: upload the scene", entry, S.wide_count, ctx->scene_wide_room);
  }
  S.needs = stack_needs(scene_wide, S.wide_depth, tree.max_depth, depth4, depth8, depth16);
  if (S.needs.need > yhk_stack_entries())
    return fail(ctx, YH_E_INVALID, "%s: BVH too deep for the traversal stack (%d > %d)", entry, S.needs.need, yhk_stack_entries());
  for (auto& n : tree.nodes) S.scene_nodes.push_back(node_lo(n)), S.scene_nodes.push_back(node_hi(n));
  S.scene_prims = tree.primitives;
  S.scene_prims.resize((S.scene_prims.size() + 3) / 4 * 4, 0);  // staged to LDS as float4
  // (a tree over the same objects has up to 2 n - 1 nodes: more than the uploaded one may have had)
  if (ctx->d_scene_nodes.bytes < S.scene_nodes.size() * 16)
    if (int rc = stage_alloc(ctx, S.d_nodes_grown, (size_t)(2 * total) * 32)) return rc;
  if (ctx->d_scene_prims.bytes < S.scene_prims.size() * 4)
    if (int rc = stage_alloc(ctx, S.d_prims_grown, S.scene_prims.size() * 4)) return rc;
  S.general_rows = general_rows_in_force(ctx);
  return YH_OK;
}

static int commit_scene_level(yh_context* ctx, SceneLevelStage& S) {
  if (S.d_nodes_grown.p) std::swap(ctx->d_scene_nodes.p, S.d_nodes_grown.p), std::swap(ctx->d_scene_nodes.bytes, S.d_nodes_grown.bytes);
  if (S.d_prims_grown.p) std::swap(ctx->d_scene_prims.p, S.d_prims_grown.p), std::swap(ctx->d_scene_prims.bytes, S.d_prims_grown.bytes);
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_nodes.p, S.scene_nodes.data(), S.scene_nodes.size() * 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_prims.p, S.scene_prims.data(), S.scene_prims.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (S.scene_wide) {  // the reserved front of the blob: zero as the upload leaves what it does not use, then the new nodes
    HIPCHK(ctx, hipMemsetAsync(ctx->d_lane_blob.p, 0, (size_t)ctx->scene_wide_room * 128, ctx->stream));
    int e = yhk_wide_collapse(2, S.nn, (const float*)S.d_stree.p, (const unsigned int*)S.d_sflag.p, (const unsigned int*)S.d_sidx.p, 1, 0, 0, ctx->d_lane_blob.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "wide collapse of the scene tree: %s", hipGetErrorString((hipError_t)e));
  }
  return YH_OK;
}

static void settle_scene_level(yh_context* ctx, const SceneLevelStage& S) {
  ctx->stack_need = S.needs.need, ctx->stack_need8 = S.needs.need8, ctx->stack_need16 = S.needs.need16;
  yhd_scene& sc = ctx->scene;
  sc.scene_nodes = (const yhd_float4*)ctx->d_scene_nodes.p, sc.scene_prims = (const int*)ctx->d_scene_prims.p;
  sc.num_scene_nodes = S.nn;
  sc.lds_scene_f4    = S.scene_wide ? 0 : S.lds_scene_f4;
  sc.scene_wide_root = S.scene_wide ? 0 : -1;
  sc.stack_entries   = std::max(8, (S.needs.need + 7) / 8 * 8);
  sc.stack_entries8  = std::max(8, (S.needs.need8 + 7) / 8 * 8);
  sc.stack_entries16 = std::max(8, (S.needs.need16 + 7) / 8 * 8);
  settle_scene_variant(ctx, sc, S.general_rows);
}

int yh_update_objects(yh_context* ctx, int first, int count, const yh_object* objects) {
  if (!ctx) return YH_E_INVALID;
  if (!objects && count != 0) return fail(ctx, YH_E_INVALID, "yh_update_objects: objects is NULL");
  if (int rc = edit_begin(ctx, "yh_update_objects")) return rc;
  const int total = ctx->scene.num_objects, num_shapes = (int)ctx->h_shape_roots.size(), num_materials = (int)ctx->h_materials.size();
  if (first < 0 || count < 0 || first > total || count > total - first)
    return fail(ctx, YH_E_INVALID, "yh_update_objects: rows [%d, %d + %d) are outside the uploaded list of %d objects", first, first, count, total);
  static_assert(sizeof(yh_object) == 56, "the fingerprint's object bytes are the rows themselves");
  bool                   lights_change = false;
  std::vector<yh_object> was((size_t)count);  // (key_geometry begins with the object rows as they were passed in)
  if (count > 0) memcpy(was.data(), ctx->key_geometry.data() + sizeof(yh_object) * (size_t)first, sizeof(yh_object) * (size_t)count);
  for (int i = 0; i < count; i++) {
    const yh_object& now = objects[i];
    if (now.shape != was[(size_t)i].shape || now.shape < 0 || now.shape >= num_shapes)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d names shape %d, the uploaded one has shape %d: upload the scene", first + i, now.shape, was[(size_t)i].shape);
    if (now.material < 0 || now.material >= num_materials)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d names material %d of %d", first + i, now.material, num_materials);
    // the light list (init_lights, pt.cpp:1695-1740) holds the objects whose material emits: the rule of yh_update_materials
    const bool black = is_black(ctx->h_materials[(size_t)now.material].emission);
    const bool toggles = black != is_black(ctx->h_materials[(size_t)was[(size_t)i].material].emission);
    lights_change = lights_change || toggles;
    if (toggles && !ctx->light_edits)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d turns its emission %s with material %d: the light list changes, upload the scene", first + i, black ? "off" : "on", now.material);
  }
  // ---- staging: the world boxes of the edited rows, from the device ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  DevBuf d_rows, d_boxes;
  static_assert(sizeof(yhh::Box) == 24, "world boxes come back as 6 floats");
  if (count > 0) {
    if (int rc = stage_alloc(ctx, d_rows, sizeof(yh_object) * (size_t)count)) return rc;
    if (int rc = stage_alloc(ctx, d_boxes, sizeof(yhh::Box) * (size_t)count)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_rows.p, objects, sizeof(yh_object) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    int e = yhk_object_rows(count, d_rows.p, (const float*)ctx->d_shape_roots.p, nullptr, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "object rows: %s", hipGetErrorString((hipError_t)e));
    HIPCHK(ctx, hipMemcpyAsync(boxes.data() + first, d_boxes.p, sizeof(yhh::Box) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    YH_WAIT(ctx);
  }
  SceneLevelStage S;
  if (int rc = stage_scene_level(ctx, "yh_update_objects", boxes, ctx->max_shape_depth, ctx->max_shape_depth8, ctx->max_shape_depth16, S)) return rc;
  LightStage LS;
  if (lights_change) {  // the light list over the edited rows
    std::vector<yh_object> rows = uploaded_rows(ctx);
    std::copy(objects, objects + count, rows.begin() + first);
    if (int rc = stage_lights(ctx, "yh_update_objects", ctx->h_materials.data(), rows.data(), emission_in_force(ctx).data(), LS)) return rc;
  }
  // ---- COMMIT ----
  ctx->have_scene = false;
  if (count > 0) {
    int e = yhk_object_rows(count, d_rows.p, (const float*)ctx->d_shape_roots.p, (yhd_object*)ctx->d_objects.p + first, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "object rows: %s", hipGetErrorString((hipError_t)e));
  }
  if (int rc = commit_scene_level(ctx, S)) return rc;
  if (lights_change)
    if (int rc = commit_lights(ctx, "yh_update_objects", LS)) return rc;
  YH_WAIT(ctx);
  if (count > 0) memcpy(ctx->key_geometry.data() + sizeof(yh_object) * (size_t)first, objects, sizeof(yh_object) * (size_t)count);
  ctx->h_obj_boxes.swap(boxes);
  settle_scene_level(ctx, S);
  ctx->have_scene = true;
  edit_end(ctx);
  return YH_OK;
}

// ---- yh_update_shape / yh_update_shape_device: set_positions / set_normals / set_radius on a shape, then init_bvh -------------------------
// (yocto_pathtrace.h:154-157). One shape's leaf records, test records, 4- / 8- / 16-wide nodes and per-vertex rows are made again with the
// upload's own code (scene_upload.cpp: build_shape_tree, index_shape_tree, collapse_shape_tree) and unit/shapes.hip; its root box moves the
// world boxes of the objects that name it, so the scene level follows as after yh_update_objects. The node counts depend on the
// positions: a width whose new count exceeds the room of the shape's region gets a new region behind the end of the traversal array
// (count + count / 8 nodes, on a multiple of 4 units), the array is reallocated and the old bytes copied device to device, the vacated
// region is zeroed and stays unused until an upload. No other shape moves: the collapse writes absolute references.
// what yh_update_shape and yh_refit_shape check of their arguments before anything is staged, and `rows`: the object list as it was passed in
// (emits: an object that names the shape is a light — refused without yh_set_light_edits, else the light list follows the edit)
static int check_shape_edit(yh_context* ctx, const char* entry, int shape, const yh_shape* now, std::vector<yh_object>& rows, bool& emits) {
  if (!now) return fail(ctx, YH_E_INVALID, "%s: now is NULL", entry);
  if (int rc = edit_begin(ctx, entry)) return rc;
  const int num_shapes = (int)ctx->shape_states.size(), total = ctx->scene.num_objects;
  if (shape < 0 || shape >= num_shapes) return fail(ctx, YH_E_INVALID, "%s: shape %d is outside the uploaded list of %d shapes", entry, shape, num_shapes);
  const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
  const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)shape];
  const bool lines = L.kind == YH_KIND_LINES;
  int was_counts[3];  // (key_geometry holds the counts as they were passed in, in front of the shape's positions)
  memcpy(was_counts, ctx->key_geometry.data() + E.key_positions - sizeof(was_counts), sizeof(was_counts));
  if ((now->num_lines > 0) != lines)
    return fail(ctx, YH_E_INVALID, "%s: shape %d was uploaded as %s and is now %s: upload the scene", entry, shape, lines ? "lines" : "triangles", lines ? "triangles" : "lines");
  if (now->num_vertices != was_counts[0] || now->num_lines != was_counts[1] || now->num_triangles != was_counts[2])
    return fail(ctx, YH_E_INVALID, "%s: shape %d has %d vertices, %d lines, %d triangles; the uploaded one has %d, %d, %d: upload the scene", entry, shape, now->num_vertices,
        now->num_lines, now->num_triangles, was_counts[0], was_counts[1], was_counts[2]);
  if (!now->positions) return fail(ctx, YH_E_INVALID, "%s: shape %d has no positions", entry, shape);
  if (!(lines ? now->lines : now->triangles)) return fail(ctx, YH_E_INVALID, "%s: shape %d has no index array", entry, shape);
  if ((now->normals != nullptr) != (E.has_normals != 0))
    return fail(ctx, YH_E_INVALID, "%s: shape %d %s normals, the uploaded one %s: upload the scene", entry, shape, now->normals ? "has" : "has no", E.has_normals ? "had them" : "had none");
  if ((now->texcoords != nullptr) != (E.has_texcoords != 0))
    return fail(ctx, YH_E_INVALID, "%s: shape %d %s texcoords, the uploaded one %s: upload the scene", entry, shape, now->texcoords ? "has" : "has no", E.has_texcoords ? "had them" : "had none");
  // the light cdf and the LDS light table (init_lights, pt.cpp:1695-1740) were made from the shape of every object whose material emits
  rows.resize((size_t)total);  // (key_geometry begins with the object rows as they were passed in)
  memcpy(rows.data(), ctx->key_geometry.data(), sizeof(yh_object) * (size_t)total);
  emits = false;
  for (int i = 0; i < total; i++) {
    if (rows[(size_t)i].shape != shape || is_black(ctx->h_materials[(size_t)rows[(size_t)i].material].emission)) continue;
    emits = !lines;  // (a line shape never is a light)
    if (!ctx->light_edits)
      return fail(ctx, YH_E_INVALID, "%s: shape %d is the shape of object %d, whose material emits: the light tables are made from it, upload the scene", entry, shape, i);
  }
  return YH_OK;
}

// ... and their staging: the arrays on the device (the host form copies them there: `dev` is the same shape with its arrays in device
// memory), the index check before anything follows an index
namespace {
struct ShapeArrays {
  DevBuf   d_pos, d_nrm, d_rad, d_idx, d_tex, d_flag;
  yh_shape dev{};
};
}  // namespace
static int stage_shape_arrays(yh_context* ctx, const char* who, int shape, const yh_shape* now, bool device, bool lines, size_t nv, size_t nidx, ShapeArrays& A) {
  const int* idx_in = lines ? now->lines : now->triangles;
  yh_shape&  dev    = A.dev;
  dev = *now;
  if (!device) {
    auto h2d = [&](DevBuf& buf, const void* src, size_t bytes, const void** to) -> int {
      if (!src) return YH_OK;
      if (int rc = stage_alloc(ctx, buf, bytes)) return rc;
      HIPCHK(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
      *to = buf.p;
      return YH_OK;
    };
    if (int rc = h2d(A.d_idx, idx_in, nidx * 4, (const void**)(lines ? &dev.lines : &dev.triangles))) return rc;
    if (int rc = h2d(A.d_pos, now->positions, nv * 12, (const void**)&dev.positions)) return rc;
    if (int rc = h2d(A.d_rad, now->radius, nv * 4, (const void**)&dev.radius)) return rc;
    if (int rc = h2d(A.d_nrm, now->normals, nv * 12, (const void**)&dev.normals)) return rc;
    if (int rc = h2d(A.d_tex, now->texcoords, nv * 8, (const void**)&dev.texcoords)) return rc;
  }
  if (int rc = stage_alloc(ctx, A.d_flag, 4)) return rc;
  int bad = 0, e = yhk_index_check((int)nidx, lines ? dev.lines : dev.triangles, now->num_vertices, (unsigned int*)A.d_flag.p, &bad, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%sindex check: %s", who, hipGetErrorString((hipError_t)e));
  if (bad) return fail(ctx, YH_E_INVALID, "%sshape %d: vertex index out of range", who, shape);
  return YH_OK;
}

int shape_slot_areas(yh_context* ctx, const char* who, int n, const yh_context::LaneShape* L, const int (*count)[3], const void* blob, double* area) {
  std::vector<int> at(3 * (size_t)n + 1, 0);  // where every (shape, width)'s partial sums begin
  for (int i = 0; i < n; i++)
    for (int w = 0; w < 3; w++) at[3 * (size_t)i + w + 1] = at[3 * (size_t)i + w] + yhk_refit_partials(count[i][w]);
  DevBuf d_part;
  if (int rc = stage_alloc(ctx, d_part, sizeof(double) * (size_t)at.back())) return rc;
  for (int i = 0; i < n; i++) {
    const long long off[3] = {L[i].node_off, L[i].node_off8, L[i].node_off16};
    for (int w = 0; w < 3; w++) {
      int e = yhk_area_partials(4 << w, blob, off[w], count[i][w], (double*)d_part.p + at[3 * (size_t)i + w], ctx->stream);
      if (e) return fail(ctx, YH_E_DEVICE, "%sslot areas: %s", who, hipGetErrorString((hipError_t)e));
    }
  }
  std::vector<double> part((size_t)at.back());
  HIPCHK(ctx, hipMemcpyAsync(part.data(), d_part.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  for (size_t j = 0; j < 3 * (size_t)n; j++) {  // the partials in index order: the same sum from run to run
    area[j] = 0;
    for (int k = at[j]; k < at[j + 1]; k++) area[j] += part[(size_t)k];
  }
  return YH_OK;
}

static int update_shape(yh_context* ctx, const char* entry, int shape, const yh_shape* now, bool device) {
  if (!ctx) return YH_E_INVALID;
  std::vector<yh_object> rows;
  bool                   emits = false;
  if (int rc = check_shape_edit(ctx, entry, shape, now, rows, emits)) return rc;
  const int num_shapes = (int)ctx->shape_states.size(), total = ctx->scene.num_objects;
  const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
  const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)shape];
  const bool lines = L.kind == YH_KIND_LINES;
  const std::string who_s = std::string(entry) + ": ";
  const char*       who   = who_s.c_str();
  const size_t nv = (size_t)now->num_vertices, nel = (size_t)L.num_prims, nidx = nel * (lines ? 2 : 3), per = lines ? 4 : 6;
  ShapeArrays A;
  if (int rc = stage_shape_arrays(ctx, who, shape, now, device, lines, nv, nidx, A)) return rc;
  const yh_shape& dev     = A.dev;
  const int*      d_index = lines ? dev.lines : dev.triangles;
  // ---- the tree, the records and the index of the wide nodes: the upload's rule for where, the upload's code ----
  const bool on_device = device || shape_builds_on_device((int)nel);
  ShapeTree  T;
  DevBuf     d_recs;
  if (int rc = stage_alloc(ctx, d_recs, nel * per * 16)) return rc;
  if (int rc = build_shape_tree(ctx, who, shape, on_device ? dev : *now, on_device, on_device, (yhd_float4*)d_recs.p, T)) return rc;
  if (int rc = index_shape_tree(ctx, who, T)) return rc;
  // ---- where the wide nodes go ----
  yh_context::LaneShape  Lnew = L;
  yh_context::ShapeState Enew = E;
  const long long old_units = ctx->scene.lane_blob_units, width[3] = {4, 8, 16}, old_off[3] = {L.node_off, L.node_off8, L.node_off16};
  long long       end = old_units, off[3] = {old_off[0], old_off[1], old_off[2]};
  for (int w = 0; w < 3; w++) {
    Enew.count[w] = T.wide_count[w];
    if (T.wide_count[w] <= E.room[w]) continue;
    off[w]       = (end + 3) / 4 * 4;
    Enew.room[w] = T.wide_count[w] + T.wide_count[w] / 8;
    end          = off[w] + width[w] * Enew.room[w] + 4;  // (four units of slack behind the last node, as the upload leaves)
  }
  if (end >= (1ll << 30)) return fail(ctx, YH_E_INVALID, "%sscene too large for 30-bit node offsets (%lld units): upload the scene", who, end);
  Lnew.num_nodes = T.wide_count[0], Lnew.node_off = off[0], Lnew.node_off8 = off[1], Lnew.node_off16 = off[2];
  Enew.depth = T.depth, Enew.depth8 = T.depth8, Enew.depth16 = T.depth16;
  DevBuf d_blob_grown;
  if (end > old_units)
    if (int rc = stage_alloc(ctx, d_blob_grown, (size_t)end * 32)) return rc;
  int depth4 = 0, depth8 = 0, depth16 = 0;
  for (int s = 0; s < num_shapes; s++) {
    const yh_context::ShapeState& D = s == shape ? Enew : ctx->shape_states[(size_t)s];
    depth4 = std::max(depth4, D.depth), depth8 = std::max(depth8, D.depth8), depth16 = std::max(depth16, D.depth16);
  }
  // ---- the world boxes of the objects that name the shape, from its new root box; the scene level over all boxes ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  std::vector<int>      named;
  for (int i = 0; i < total; i++)
    if (rows[(size_t)i].shape == shape) named.push_back(i);
  DevBuf d_rows, d_boxes, d_named, d_root;
  if (int rc = stage_alloc(ctx, d_rows, sizeof(yh_object) * (size_t)total)) return rc;
  if (int rc = stage_alloc(ctx, d_boxes, sizeof(yhh::Box) * (size_t)total)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(d_rows.p, rows.data(), sizeof(yh_object) * (size_t)total, hipMemcpyHostToDevice, ctx->stream));
  std::vector<yh_object> named_rows;  // (their shape is row 0 of a table of one root box: the context's table changes at COMMIT only)
  std::vector<yhh::Box>  named_boxes(named.size());
  for (int i : named) named_rows.push_back(rows[(size_t)i]), named_rows.back().shape = 0;
  if (!named.empty()) {
    if (int rc = stage_alloc(ctx, d_named, sizeof(yh_object) * named.size())) return rc;
    if (int rc = stage_alloc(ctx, d_root, sizeof(yhh::Box))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_named.p, named_rows.data(), sizeof(yh_object) * named.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_root.p, &T.root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
    int e = yhk_object_rows((int)named.size(), d_named.p, (const float*)d_root.p, nullptr, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
    HIPCHK(ctx, hipMemcpyAsync(named_boxes.data(), d_boxes.p, sizeof(yhh::Box) * named.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  // the fingerprint's bytes of the shape: its first and last 256 positions (the device form fetches them)
  const size_t take = std::min<size_t>(nv, 256);
  std::vector<unsigned char> key_bytes(2 * take * 12);
  if (device) {
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data(), dev.positions, take * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data() + take * 12, dev.positions + 3 * (nv - take), take * 12, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    memcpy(key_bytes.data(), now->positions, take * 12), memcpy(key_bytes.data() + take * 12, now->positions + 3 * (nv - take), take * 12);
  }
  YH_WAIT(ctx);
  for (size_t k = 0; k < named.size(); k++) boxes[(size_t)named[k]] = named_boxes[k];
  SceneLevelStage S;
  if (int rc = stage_scene_level(ctx, entry, boxes, depth4, depth8, depth16, S)) return rc;
  LightStage LS;  // an emitter's shape: the cdf and the record of the lights that name it, made once the new arrays sit in the context's rows
  if (emits)
    if (int rc = stage_lights_of_shape(ctx, shape, rows.data(), LS)) return rc;
  // ---- COMMIT: from here on kernels, copies and memsets only ----
  ctx->have_scene = false;
  if (d_blob_grown.p) {  // the old array's bytes as they are, zeros behind them (what alloc_zero leaves)
    HIPCHK(ctx, hipMemcpyAsync(d_blob_grown.p, ctx->d_lane_blob.p, (size_t)old_units * 32, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync((char*)d_blob_grown.p + (size_t)old_units * 32, 0, (size_t)(end - old_units) * 32, ctx->stream));
    std::swap(ctx->d_lane_blob.p, d_blob_grown.p), std::swap(ctx->d_lane_blob.bytes, d_blob_grown.bytes);
    ctx->scene.lane_blob = nullptr;
  }
  for (int w = 0; w < 3; w++)  // the shape's regions as they were: vacated, or written again with the unused rest zero
    if (E.room[w] > 0) HIPCHK(ctx, hipMemsetAsync((char*)ctx->d_lane_blob.p + (size_t)old_off[w] * 32, 0, (size_t)(width[w] * E.room[w]) * 32, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync((yhd_float4*)ctx->d_prims.p + L.prim_base, d_recs.p, nel * per * 16, hipMemcpyDeviceToDevice, ctx->stream));
  if (int rc = collapse_shape_tree(ctx, who, T, Lnew, ctx->d_lane_blob.p)) return rc;
  if (E.per_vertex) {
    int e = yhk_vertex_rows(lines ? 1 : 0, (int)nv, (int)nel, dev.positions, dev.radius, dev.texcoords, d_index, (yhd_float4*)ctx->d_vpos.p + E.vert_base,
        (float*)ctx->d_vtex.p + 2 * (size_t)E.vert_base, (yhd_int4*)ctx->d_elems.p + E.elem_base, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%svertex rows: %s", who, hipGetErrorString((hipError_t)e));
  }
  HIPCHK(ctx, hipMemcpyAsync((yhh::Box*)ctx->d_shape_roots.p + shape, &T.root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
  {  // the rows of the objects that name the shape, run by run of consecutive ones (no other object's row is written), then the lane roots
    int e = 0;
    for (size_t k = 0; k < named.size() && !e;) {
      size_t end_k = k + 1;
      while (end_k < named.size() && named[end_k] == named[end_k - 1] + 1) end_k++;
      const int first = named[k], run = (int)(end_k - k);
      e = yhk_object_rows(run, (const yh_object*)d_rows.p + first, (const float*)ctx->d_shape_roots.p, (yhd_object*)ctx->d_objects.p + first, (float*)d_boxes.p + 6 * (size_t)first, ctx->stream);
      k = end_k;
    }
    if (!e) e = yhk_object_lane_roots(total, d_rows.p, shape, (int)Lnew.node_off, (int)Lnew.node_off8, (int)Lnew.node_off16, ctx->d_objects.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
  }
  if (int rc = commit_scene_level(ctx, S)) return rc;
  if (emits)
    if (int rc = commit_lights_of_shape(ctx, entry, LS)) return rc;
  YH_WAIT(ctx);
  memcpy(ctx->key_geometry.data() + E.key_positions, key_bytes.data(), key_bytes.size());
  ctx->scene.num_nodes_total += T.wide_count[0] - E.count[0];
  for (int w = 0; w < 3; w++) {
    Enew.wide_levels[w] = T.wide_levels[w];
    memcpy(Enew.wide_first[w], T.wide_first[w], sizeof(Enew.wide_first[w]));
  }
  if (int rc = shape_slot_areas(ctx, who, 1, &Lnew, &Enew.count, ctx->d_lane_blob.p, Enew.area_build)) return rc;
  memcpy(Enew.area_now, Enew.area_build, sizeof(Enew.area_now));
  ctx->lane_shapes[(size_t)shape]  = Lnew;
  ctx->shape_states[(size_t)shape] = Enew;  // (E and L are these: not read below)
  ctx->lane_units = 0;
  for (int s = 0; s < num_shapes; s++)  // the end of the furthest 4-wide region: what the one-lane kernels address
    ctx->lane_units = std::max(ctx->lane_units, ctx->lane_shapes[(size_t)s].node_off + 4ll * ctx->shape_states[(size_t)s].room[0] + 4);
  ctx->scene.lane_blob = (const yhd_float4*)ctx->d_lane_blob.p, ctx->scene.lane_blob_units = end;
  ctx->h_shape_roots[(size_t)shape] = T.root;
  ctx->h_obj_boxes.swap(boxes);
  ctx->max_shape_depth = depth4, ctx->max_shape_depth8 = depth8, ctx->max_shape_depth16 = depth16;
  settle_scene_level(ctx, S);
  ctx->have_scene = true;
  edit_end(ctx);
  return YH_OK;
}

int yh_update_shape(yh_context* ctx, int shape, const yh_shape* now) { return update_shape(ctx, "yh_update_shape", shape, now, false); }
int yh_update_shape_device(yh_context* ctx, int shape, const yh_shape* now) { return update_shape(ctx, "yh_update_shape_device", shape, now, true); }

// ---- yh_refit_shape / yh_refit_shape_device: the same edit, kept in the tree the shape's last build left (unit/refit.hip) ------------------
// Nothing is built: the leaf slots keep their elements (a record holds its element id), so the records are written again where they are,
// the test records made from them, and the boxes of the 4- / 8- / 16-wide nodes recomputed bottom-up in place, one launch per level of
// each wide tree (ShapeState::wide_first). The traversal array neither grows nor moves, the depths stay. What can refuse runs first: the
// checks, the index check, the new root box (a min / max reduction over the primitive boxes) and the scene level over the world boxes
// that follow from it. The only scratch the shape sizes: its primitive boxes in leaf order, and the host form's staged arrays.
static int refit_shape(yh_context* ctx, const char* entry, int shape, const yh_shape* now, bool device) {
  if (!ctx) return YH_E_INVALID;
  std::vector<yh_object> rows;
  bool                   emits = false;
  if (int rc = check_shape_edit(ctx, entry, shape, now, rows, emits)) return rc;
  const int total = ctx->scene.num_objects;
  yh_context::ShapeState&      E = ctx->shape_states[(size_t)shape];
  const yh_context::LaneShape& L = ctx->lane_shapes[(size_t)shape];
  const bool lines = L.kind == YH_KIND_LINES;
  const std::string who_s = std::string(entry) + ": ";
  const char*       who   = who_s.c_str();
  const size_t nv = (size_t)now->num_vertices, nel = (size_t)L.num_prims, nidx = nel * (lines ? 2 : 3);
  ShapeArrays A;
  if (int rc = stage_shape_arrays(ctx, who, shape, now, device, lines, nv, nidx, A)) return rc;
  const yh_shape& dev     = A.dev;
  const int*      d_index = lines ? dev.lines : dev.triangles;
  yhd_float4*     d_recs  = (yhd_float4*)ctx->d_prims.p + L.prim_base;
  // ---- the primitive boxes in leaf order and their union, the shape's new root box ----
  const int parts = yhk_refit_partials((int)nel);
  DevBuf    d_lboxes, d_part;
  if (int rc = stage_alloc(ctx, d_lboxes, nel * sizeof(yhh::Box))) return rc;
  if (int rc = stage_alloc(ctx, d_part, sizeof(yhh::Box) * (size_t)parts)) return rc;
  int e = yhk_refit_boxes(lines ? 1 : 0, (int)nel, d_recs, dev.positions, dev.radius, d_index, (float*)d_lboxes.p, ctx->stream);
  if (!e) e = yhk_box_partials((int)nel, (const float*)d_lboxes.p, (float*)d_part.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%sprimitive bounds: %s", who, hipGetErrorString((hipError_t)e));
  std::vector<yhh::Box> part((size_t)parts);
  HIPCHK(ctx, hipMemcpyAsync(part.data(), d_part.p, sizeof(yhh::Box) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  // the fingerprint's bytes of the shape: its first and last 256 positions (the device form fetches them)
  const size_t take = std::min<size_t>(nv, 256);
  std::vector<unsigned char> key_bytes(2 * take * 12);
  if (device) {
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data(), dev.positions, take * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data() + take * 12, dev.positions + 3 * (nv - take), take * 12, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    memcpy(key_bytes.data(), now->positions, take * 12), memcpy(key_bytes.data() + take * 12, now->positions + 3 * (nv - take), take * 12);
  }
  YH_WAIT(ctx);
  yhh::Box root = part[0];
  for (int k = 1; k < parts; k++)
    for (int c = 0; c < 3; c++) root.min[c] = fmin_(root.min[c], part[(size_t)k].min[c]), root.max[c] = fmax_(root.max[c], part[(size_t)k].max[c]);
  // ---- the world boxes of the objects that name the shape, from its new root box; the scene level over all boxes ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  std::vector<int>      named;
  for (int i = 0; i < total; i++)
    if (rows[(size_t)i].shape == shape) named.push_back(i);
  DevBuf d_rows, d_boxes, d_named, d_root;
  if (int rc = stage_alloc(ctx, d_rows, sizeof(yh_object) * (size_t)total)) return rc;
  if (int rc = stage_alloc(ctx, d_boxes, sizeof(yhh::Box) * (size_t)total)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(d_rows.p, rows.data(), sizeof(yh_object) * (size_t)total, hipMemcpyHostToDevice, ctx->stream));
  std::vector<yh_object> named_rows;  // (their shape is row 0 of a table of one root box: the context's table changes at COMMIT only)
  std::vector<yhh::Box>  named_boxes(named.size());
  for (int i : named) named_rows.push_back(rows[(size_t)i]), named_rows.back().shape = 0;
  if (!named.empty()) {
    if (int rc = stage_alloc(ctx, d_named, sizeof(yh_object) * named.size())) return rc;
    if (int rc = stage_alloc(ctx, d_root, sizeof(yhh::Box))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_named.p, named_rows.data(), sizeof(yh_object) * named.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_root.p, &root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
    e = yhk_object_rows((int)named.size(), d_named.p, (const float*)d_root.p, nullptr, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
    HIPCHK(ctx, hipMemcpyAsync(named_boxes.data(), d_boxes.p, sizeof(yhh::Box) * named.size(), hipMemcpyDeviceToHost, ctx->stream));
    YH_WAIT(ctx);
  }
  for (size_t k = 0; k < named.size(); k++) boxes[(size_t)named[k]] = named_boxes[k];
  SceneLevelStage S;
  if (int rc = stage_scene_level(ctx, entry, boxes, ctx->max_shape_depth, ctx->max_shape_depth8, ctx->max_shape_depth16, S)) return rc;
  LightStage LS;  // an emitter's shape: the cdf and the record of the lights that name it (the cdf is by element: it does not depend on the tree)
  if (emits)
    if (int rc = stage_lights_of_shape(ctx, shape, rows.data(), LS)) return rc;
  // ---- COMMIT: from here on kernels and copies only ----
  ctx->have_scene = false;
  e = yhk_refit_records(lines ? 1 : 0, (int)nel, dev.positions, dev.normals, dev.radius, d_index, d_recs, ctx->stream);
  if (!e) e = yhk_lane_tests((const yhd_float4*)ctx->d_prims.p, (yhd_float4*)ctx->d_lane_blob.p, L.kind, L.prim_base, L.num_prims, L.test_off, ctx->stream);
  const long long offs[3] = {L.node_off, L.node_off8, L.node_off16};
  for (int w = 0; w < 3 && !e; w++)
    e = yhk_refit_wide(2 + w, ctx->d_lane_blob.p, offs[w], L.test_off, lines ? 1 : 2, E.wide_levels[w], E.wide_first[w], (const float*)d_lboxes.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%srefit: %s", who, hipGetErrorString((hipError_t)e));
  if (E.per_vertex) {
    e = yhk_vertex_rows(lines ? 1 : 0, (int)nv, (int)nel, dev.positions, dev.radius, dev.texcoords, d_index, (yhd_float4*)ctx->d_vpos.p + E.vert_base,
        (float*)ctx->d_vtex.p + 2 * (size_t)E.vert_base, (yhd_int4*)ctx->d_elems.p + E.elem_base, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%svertex rows: %s", who, hipGetErrorString((hipError_t)e));
  }
  HIPCHK(ctx, hipMemcpyAsync((yhh::Box*)ctx->d_shape_roots.p + shape, &root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
  e = 0;  // the rows of the objects that name the shape, run by run of consecutive ones (their lane roots stay: nothing moved)
  for (size_t k = 0; k < named.size() && !e;) {
    size_t end_k = k + 1;
    while (end_k < named.size() && named[end_k] == named[end_k - 1] + 1) end_k++;
    const int first = named[k], run = (int)(end_k - k);
    e = yhk_object_rows(run, (const yh_object*)d_rows.p + first, (const float*)ctx->d_shape_roots.p, (yhd_object*)ctx->d_objects.p + first, (float*)d_boxes.p + 6 * (size_t)first, ctx->stream);
    k = end_k;
  }
  if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
  if (int rc = commit_scene_level(ctx, S)) return rc;
  if (emits)
    if (int rc = commit_lights_of_shape(ctx, entry, LS)) return rc;
  double area[3];
  if (int rc = shape_slot_areas(ctx, who, 1, &L, &E.count, ctx->d_lane_blob.p, area)) return rc;  // (waits for the stream)
  memcpy(E.area_now, area, sizeof(area));
  memcpy(ctx->key_geometry.data() + E.key_positions, key_bytes.data(), key_bytes.size());
  ctx->h_shape_roots[(size_t)shape] = root;
  ctx->h_obj_boxes.swap(boxes);
  settle_scene_level(ctx, S);
  ctx->have_scene = true;
  edit_end(ctx);
  return YH_OK;
}

int yh_refit_shape(yh_context* ctx, int shape, const yh_shape* now) { return refit_shape(ctx, "yh_refit_shape", shape, now, false); }
int yh_refit_shape_device(yh_context* ctx, int shape, const yh_shape* now) { return refit_shape(ctx, "yh_refit_shape_device", shape, now, true); }

int yh_set_light_edits(yh_context* ctx, int on) {
  if (!ctx) return YH_E_INVALID;
  ctx->light_edits = on != 0;
  return YH_OK;
}

int yh_light_list(const yh_context* ctx, int* object, int* environment, int* cdf_count, int* in_lds, int capacity) {
  if (!ctx) return YH_E_INVALID;
  if (!ctx->have_scene) return YH_E_STATE;
  const yhd_scene& sc = ctx->scene;
  for (int i = 0; i < sc.num_lights && i < capacity; i++) {
    if (object) object[i] = sc.lights[i].object;
    if (environment) environment[i] = sc.lights[i].environment;
    if (cdf_count) cdf_count[i] = sc.lights[i].cdf_count;
    if (in_lds) in_lds[i] = sc.lights[i].small_base >= 0;
  }
  return sc.num_lights;
}

// init_lights' area cdf of one triangle shape (pt.cpp:1695-1740): the upload's loop restated, and the kernel of the edit
static bool triangle_cdf_args(int num_vertices, const float* positions, int num_triangles, const int* triangles, const float* cdf) {
  if (num_vertices <= 0 || num_triangles <= 0 || !positions || !triangles || !cdf) return false;
  for (size_t k = 0; k < 3 * (size_t)num_triangles; k++)
    if (triangles[k] < 0 || triangles[k] >= num_vertices) return false;
  return true;
}

int yh_triangle_cdf(int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf) {
  if (!triangle_cdf_args(num_vertices, positions, num_triangles, triangles, cdf)) return YH_E_INVALID;
  for (int t = 0; t < num_triangles; t++) {
    float area = triangle_area(ld3(positions + 3 * (size_t)triangles[3 * t]), ld3(positions + 3 * (size_t)triangles[3 * t + 1]), ld3(positions + 3 * (size_t)triangles[3 * t + 2]));
    if (t) area += cdf[t - 1];
    cdf[t] = area;
  }
  return YH_OK;
}

int yh_triangle_cdf_gpu(yh_context* ctx, int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf) {
  if (!ctx) return YH_E_INVALID;
  if (!triangle_cdf_args(num_vertices, positions, num_triangles, triangles, cdf))
    return fail(ctx, YH_E_INVALID, "yh_triangle_cdf_gpu: a NULL array, an empty shape or a vertex index outside [0, %d)", num_vertices);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->poisoned) return fail(ctx, YH_E_DEVICE, "a launch of this context exceeded its deadline: the context refuses further work, destroy it");
  YH_WAIT(ctx);
  const yhk_light_job job{0, 0, num_triangles, 0, 0, 0, -1, 0};
  DevBuf d_job, d_pos, d_tri, d_cdf;
  if (int rc = stage_alloc(ctx, d_job, sizeof(job))) return rc;
  if (int rc = stage_alloc(ctx, d_pos, (size_t)num_vertices * 12)) return rc;
  if (int rc = stage_alloc(ctx, d_tri, (size_t)num_triangles * 12)) return rc;
  if (int rc = stage_alloc(ctx, d_cdf, (size_t)num_triangles * 4)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(d_job.p, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_pos.p, positions, (size_t)num_vertices * 12, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_tri.p, triangles, (size_t)num_triangles * 12, hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_triangle_cdf_raw(d_job.p, (const float*)d_pos.p, (const int*)d_tri.p, (float*)d_cdf.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "yh_triangle_cdf_gpu: %s", hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(cdf, d_cdf.p, (size_t)num_triangles * 4, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  return YH_OK;
}

int yh_shape_refit_growth(const yh_context* ctx, int shape, float growth[3]) {
  if (!ctx) return YH_E_INVALID;
  if (!ctx->have_scene) return YH_E_STATE;
  if (shape < 0 || shape >= (int)ctx->shape_states.size() || !growth) return YH_E_INVALID;
  const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
  for (int w = 0; w < 3; w++) growth[w] = E.area_now[w] == E.area_build[w] ? 1.0f : (float)(E.area_now[w] / E.area_build[w]);
  return YH_OK;
}

int yh_shape_nodes(const yh_context* ctx, int shape, int64_t offset[3], int count[3], int room[3]) {
  if (!ctx) return YH_E_INVALID;
  if (!ctx->have_scene) return YH_E_STATE;
  if (shape < 0 || shape >= (int)ctx->shape_states.size() || !offset || !count || !room) return YH_E_INVALID;
  const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)shape];
  const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
  offset[0] = L.node_off, offset[1] = L.node_off8, offset[2] = L.node_off16;
  for (int w = 0; w < 3; w++) count[w] = E.count[w], room[w] = E.room[w];
  return YH_OK;
}

int yh_download_display(yh_context* ctx, float exposure, int filmic, int srgb, uint8_t* rgba8) {
  if (!ctx) return YH_E_INVALID;
  if (!rgba8) return fail(ctx, YH_E_INVALID, "yh_download_display: rgba8 is NULL");
  if (ctx->poisoned) return fail(ctx, YH_E_DEVICE, "a launch of this context exceeded its deadline: the context refuses further work, destroy it");
  if (!ctx->have_state) return fail(ctx, YH_E_STATE, "yh_download_display before yh_init_state");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->state.width * ctx->state.height * 4;
  if (!ctx->d_display.p || ctx->d_display.bytes < bytes) {
    YH_WAIT(ctx);
    ctx->d_display.reset();
    HIPCHK(ctx, hipMalloc(&ctx->d_display.p, std::max<size_t>(bytes, 16)));
    ctx->d_display.bytes = std::max<size_t>(bytes, 16);
  }
  int e = yhk_display(&ctx->state, ctx->state.samples_done, exposure, filmic ? 1 : 0, srgb ? 1 : 0, ctx->d_display.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "k_display launch: %s", hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(rgba8, ctx->d_display.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  return YH_OK;
}
