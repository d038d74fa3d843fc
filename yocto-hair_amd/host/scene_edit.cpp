// scene_edit.cpp — edits of an uploaded scene that keep its geometry: the camera, rows of the material table, the environments' frames and
// emission, and rows of the object list (yh_update_objects: it builds the scene-level tree over the objects' world boxes again). The
// reference reads its scene structs live (an interactive caller edits app->camera->frame and traces on,
// apps/ysceneitraces/ysceneitraces.cpp:392-410); here the description was flattened at yh_upload_scene, so an edit is a call of its own
// that leaves the context as an upload of the edited description would: the scene table, the material rows on the device, the kernel
// variant, the once-per-ray form, the fingerprint and the launch planning. Nothing here reads, writes or allocates anything the geometry
// sizes. How every edit begins and ends, and the scene level again, are shared with the shape edits (shape_edit.cpp); where one of
// these edits changes the light list, light_edit.cpp makes it again (edit_internal.h).
#include "edit_internal.h"

int edit_begin(yh_context* ctx, const char* entry) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->poisoned) return refuse_poisoned(ctx);
  if (!ctx->have_scene) return fail(ctx, YH_E_STATE, "%s before yh_upload_scene", entry);
  YH_WAIT(ctx);  // (an asynchronous launch may still be reading the tables this call rewrites: wait for it, within the deadline)
  return YH_OK;
}
void edit_end(yh_context* ctx) {  // the image state is gone and the next yh_init_state probes and plans as for a new scene
  ctx->scene_key = scene_fingerprint(ctx);
  forget_image_of_scene(ctx);
}

bool general_rows_in_force(const yh_context* ctx) {
  const bool                mapped = !ctx->h_maps.empty();
  const int                 n      = (int)ctx->h_materials.size();
  std::vector<yhd_material> rows((size_t)n);
  std::vector<yhd_maps>     dmaps(mapped ? (size_t)n : 0);
  return make_material_rows(ctx->h_materials.data(), mapped ? ctx->h_maps.data() : nullptr, n, rows.data(), dmaps.data());
}
std::vector<yh_object> uploaded_rows(const yh_context* ctx) {  // (key_geometry begins with them)
  static_assert(sizeof(yh_object) == 56, "the fingerprint's object bytes are the rows themselves");
  std::vector<yh_object> rows((size_t)ctx->scene.num_objects);
  memcpy(rows.data(), ctx->key_geometry.data(), sizeof(yh_object) * rows.size());
  return rows;
}
std::vector<float> emission_in_force(const yh_context* ctx) {
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
  temporal_drop(ctx);  // (other materials: the temporal history shows another lighting)
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
  temporal_drop(ctx);
  edit_end(ctx);
  return YH_OK;
}

// ---- the scene level again: what yh_update_objects and the shape edits share (edit_internal.h) --------------------------------------------
int stage_scene_level(yh_context* ctx, const char* entry, const std::vector<yhh::Box>& boxes, int depth4, int depth8, int depth16, SceneLevelStage& S) {
  const int         total = ctx->scene.num_objects;
  const std::string who   = std::string(entry) + ": ";
  if (int rc = derive_scene_level(ctx, who.c_str(), boxes, total, depth4, depth8, depth16, S)) return rc;
  if (S.scene_wide != (ctx->scene.scene_wide_root >= 0))
    return fail(ctx, YH_E_INVALID, "%s: the scene tree of the moved objects has %d nodes and its scene level %s: room for wide scene nodes exists only where the upload put it, upload the scene",
        entry, S.nn, S.scene_wide ? "no longer fits the kernels' table (it would be walked as 4-wide nodes)" : "fits the kernels' table again (it was uploaded as 4-wide nodes)");
  if (S.wide_count > ctx->scene_wide_room)
    return fail(ctx, YH_E_INVALID, "%s: %d wide scene nodes, the upload left room for %d: upload the scene", entry, S.wide_count, ctx->scene_wide_room);
  if (int rc = check_stack_needs(ctx, who.c_str(), S.needs)) return rc;
  // (a tree over the same objects has up to 2 n - 1 nodes: more than the uploaded one may have had)
  if (ctx->d_scene_nodes.bytes < S.scene_nodes.size() * 16)
    if (int rc = dev_alloc(ctx, S.d_nodes_grown, (size_t)(2 * total) * 32)) return rc;
  if (ctx->d_scene_prims.bytes < S.scene_prims.size() * 4)
    if (int rc = dev_alloc(ctx, S.d_prims_grown, S.scene_prims.size() * 4)) return rc;
  S.general_rows = general_rows_in_force(ctx);
  return YH_OK;
}

int commit_scene_level(yh_context* ctx, SceneLevelStage& S) {
  if (S.d_nodes_grown.p) ctx->d_scene_nodes.swap(S.d_nodes_grown);
  if (S.d_prims_grown.p) ctx->d_scene_prims.swap(S.d_prims_grown);
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_nodes.p, S.scene_nodes.data(), S.scene_nodes.size() * 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_prims.p, S.scene_prims.data(), S.scene_prims.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (S.scene_wide)  // the reserved front of the blob: zero as the upload leaves what it does not use, then the new nodes
    HIPCHK(ctx, hipMemsetAsync(ctx->d_lane_blob.p, 0, (size_t)ctx->scene_wide_room * 128, ctx->stream));
  return collapse_scene_tree(ctx, S, ctx->d_lane_blob.p);
}

void settle_scene_level(yh_context* ctx, const SceneLevelStage& S) {
  set_scene_level_fields(ctx, ctx->scene, S);
  settle_scene_variant(ctx, ctx->scene, S.general_rows);
}

// ---- yh_update_objects: set_frame / set_material on an object (yocto_pathtrace.h:110-111) ------------------------------------------------
// Shape trees live in object space, so a moved object changes its row (frame, inverse, padded world box, material), the reference's scene
// tree over the world boxes and what follows from that tree: the table sizes, the 4-wide scene nodes at the front of the lane blob, the
// stack needs, the kernel variant. The per-object arithmetic runs on the device (unit/objects.hip), the tree is built as the upload
// builds it (yhh::build_bvh on the host, the device's collapse). Everything that can refuse is computed into staging first; from COMMIT
// on only copies, a memset and two kernels run, and an error there leaves the context without a scene, as a failed upload does.
int yh_update_objects(yh_context* ctx, int first, int count, const yh_object* objects) {
  if (!ctx) return YH_E_INVALID;
  if (!objects && count != 0) return fail(ctx, YH_E_INVALID, "yh_update_objects: objects is NULL");
  if (int rc = edit_begin(ctx, "yh_update_objects")) return rc;
  const int total = ctx->scene.num_objects, num_shapes = (int)ctx->h_shape_roots.size(), num_materials = (int)ctx->h_materials.size();
  if (first < 0 || count < 0 || first > total || count > total - first)
    return fail(ctx, YH_E_INVALID, "yh_update_objects: rows [%d, %d + %d) are outside the uploaded list of %d objects", first, first, count, total);
  bool                   lights_change = false;
  std::vector<yh_object> rows = uploaded_rows(ctx);  // every row as it was; the edited ones are written over below
  for (int i = 0; i < count; i++) {
    const yh_object &now = objects[i], &was = rows[(size_t)first + i];
    if (now.shape != was.shape || now.shape < 0 || now.shape >= num_shapes)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d names shape %d, the uploaded one has shape %d: upload the scene", first + i, now.shape, was.shape);
    if (now.material < 0 || now.material >= num_materials)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d names material %d of %d", first + i, now.material, num_materials);
    // the light list (init_lights, pt.cpp:1695-1740) holds the objects whose material emits: the rule of yh_update_materials
    const bool black = is_black(ctx->h_materials[(size_t)now.material].emission);
    const bool toggles = black != is_black(ctx->h_materials[(size_t)was.material].emission);
    lights_change = lights_change || toggles;
    if (toggles && !ctx->light_edits)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: object %d turns its emission %s with material %d: the light list changes, upload the scene", first + i, black ? "off" : "on", now.material);
  }
  // ---- staging: the world boxes of the edited rows, from the device ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  DevBuf d_rows, d_boxes;
  static_assert(sizeof(yhh::Box) == 24, "world boxes come back as 6 floats");
  if (count > 0) {
    if (int rc = dev_alloc(ctx, d_rows, sizeof(yh_object) * (size_t)count)) return rc;
    if (int rc = dev_alloc(ctx, d_boxes, sizeof(yhh::Box) * (size_t)count)) return rc;
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
  for (int i = 0; i < count; i++)  // (an object with another material: its pixels of the temporal history are not reused)
    if (objects[i].material != rows[(size_t)first + i].material || lights_change) temporal_mark_object(ctx, first + i);
  if (count > 0) memcpy(ctx->key_geometry.data() + sizeof(yh_object) * (size_t)first, objects, sizeof(yh_object) * (size_t)count);
  ctx->h_obj_boxes.swap(boxes);
  settle_scene_level(ctx, S);
  ctx->have_scene = true;
  edit_end(ctx);
  return YH_OK;
}
