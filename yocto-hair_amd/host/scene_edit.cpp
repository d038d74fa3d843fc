// scene_edit.cpp — edits of an uploaded scene that leave every shape's acceleration structure as it is: the camera, rows of the material
// table, the environments' frames and emission, and rows of the object list (yh_update_objects, at the end: the one edit that builds
// something, the scene-level tree over the objects' world boxes). The reference reads its scene structs live (an interactive caller edits app->camera->frame and traces
// on, apps/ysceneitraces/ysceneitraces.cpp:392-410); here the description was flattened at yh_upload_scene, so an edit is a call of its own
// that leaves the context as an upload of the edited description would: the scene table, the material rows on the device, the kernel
// variant, the once-per-ray form, the fingerprint and the launch planning. Nothing the geometry sizes is read, written or allocated.
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
  for (int i = 0; i < count; i++) {
    const yh_material &was = ctx->h_materials[(size_t)first + i], &now = materials[i];
    // the light list (init_lights, pt.cpp:1695-1740) was made from the shapes' host arrays, which were borrowed for the upload only
    if (is_black(was.emission) != is_black(now.emission))
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
  if (count > 0)
    HIPCHK(ctx, hipMemcpy((yhd_material*)ctx->d_materials.p + first, rows.data() + first, sizeof(yhd_material) * (size_t)count, hipMemcpyHostToDevice));
  if (mapped && count > 0)  // (a map's record carries the material's opacity before its snap)
    HIPCHK(ctx, hipMemcpy((yhd_maps*)ctx->d_maps.p + first, dmaps.data() + first, sizeof(yhd_maps) * (size_t)count, hipMemcpyHostToDevice));
  ctx->h_materials.swap(all);
  if (mapped) ctx->h_dmaps.swap(dmaps);
  settle_scene_variant(ctx, ctx->scene, general_rows);
  edit_end(ctx);
  return YH_OK;
}

int yh_update_environments(yh_context* ctx, int count, const yh_environment* environments) {
  if (!ctx) return YH_E_INVALID;
  if (!environments && count != 0) return fail(ctx, YH_E_INVALID, "yh_update_environments: environments is NULL");
  if (int rc = edit_begin(ctx, "yh_update_environments")) return rc;
  if (count != ctx->scene.num_environments)
    return fail(ctx, YH_E_INVALID, "yh_update_environments: %d environments, the uploaded scene has %d", count, ctx->scene.num_environments);
  for (int i = 0; i < count; i++)
    if (is_black(ctx->scene.environments[i].emission) != is_black(environments[i].emission))
      return fail(ctx, YH_E_INVALID, "yh_update_environments: environment %d turns its emission %s: the light list changes, upload the scene", i, is_black(environments[i].emission) ? "off" : "on");
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
static int stage_alloc(yh_context* ctx, DevBuf& buf, size_t bytes) {
  buf.reset();
  HIPCHK(ctx, hipMalloc(&buf.p, std::max<size_t>(bytes, 16)));
  buf.bytes = std::max<size_t>(bytes, 16);
  return YH_OK;
}

int yh_update_objects(yh_context* ctx, int first, int count, const yh_object* objects) {
  if (!ctx) return YH_E_INVALID;
  if (!objects && count != 0) return fail(ctx, YH_E_INVALID, "yh_update_objects: objects is NULL");
  if (int rc = edit_begin(ctx, "yh_update_objects")) return rc;
  const int total = ctx->scene.num_objects, num_shapes = (int)ctx->h_shape_roots.size(), num_materials = (int)ctx->h_materials.size();
  if (first < 0 || count < 0 || first > total || count > total - first)
    return fail(ctx, YH_E_INVALID, "yh_update_objects: rows [%d, %d + %d) are outside the uploaded list of %d objects", first, first, count, total);
  static_assert(sizeof(yh_object) == 56, "the fingerprint's object bytes are the rows themselves");
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
    if (black != is_black(ctx->h_materials[(size_t)was[(size_t)i].material].emission))
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
  // ---- the scene-level tree, as the upload builds it, and what the upload derives from it ----
  yhh::Tree tree;
  yhh::build_bvh(tree, boxes);
  const int  nn = (int)tree.nodes.size();
  int        lds_scene_f4 = 0;
  const bool scene_wide = scene_level_is_wide(total, nn, &lds_scene_f4), was_wide = ctx->scene.scene_wide_root >= 0;
  if (scene_wide != was_wide)
    return fail(ctx, YH_E_INVALID, "yh_update_objects: the scene tree of the moved objects has %d nodes and its scene level %s: room for wide scene nodes exists only where the upload put it, upload the scene",
        nn, scene_wide ? "no longer fits the kernels' table (it would be walked as 4-wide nodes)" : "fits the kernels' table again (it was uploaded as 4-wide nodes)");
  DevBuf d_stree, d_sflag, d_sidx;
  int    wide_count = 0, wide_depth = 0;
  if (scene_wide) {
    int levels = 1, level_first[130] = {0};
    if (!tree_levels(tree, levels, level_first)) return fail(ctx, YH_E_INVALID, "yh_update_objects: scene tree of %d levels", levels);
    if (int rc = stage_alloc(ctx, d_stree, (size_t)nn * 32)) return rc;
    if (int rc = stage_alloc(ctx, d_sflag, ((size_t)nn + 1) * 4)) return rc;
    if (int rc = stage_alloc(ctx, d_sidx, ((size_t)nn + 1) * 4)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_stree.p, tree.nodes.data(), (size_t)nn * 32, hipMemcpyHostToDevice, ctx->stream));
    int e = yhk_wide_index(nn, (const float*)d_stree.p, levels, level_first, 2, (unsigned int*)d_sflag.p, (unsigned int*)d_sidx.p, &wide_count, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "wide-node index of the scene tree: %s", hipGetErrorString((hipError_t)e));
    wide_depth = 1 + std::max(0, levels - 2) / 2;
    if (wide_count > ctx->scene_wide_room)
      return fail(ctx, YH_E_INVALID, "yh_update_objects: %d wide scene nodes, the upload left room for %d: upload the scene", wide_count, ctx->scene_wide_room);
  }
  const StackNeeds needs = stack_needs(scene_wide, wide_depth, tree.max_depth, ctx->max_shape_depth, ctx->max_shape_depth8, ctx->max_shape_depth16);
  if (needs.need > yhk_stack_entries())
    return fail(ctx, YH_E_INVALID, "yh_update_objects: BVH too deep for the traversal stack (%d > %d)", needs.need, yhk_stack_entries());
  std::vector<yhd_float4> scene_nodes;
  for (auto& n : tree.nodes) scene_nodes.push_back(node_lo(n)), scene_nodes.push_back(node_hi(n));
  std::vector<int> scene_prims = tree.primitives;
  scene_prims.resize((scene_prims.size() + 3) / 4 * 4, 0);  // staged to LDS as float4
  DevBuf d_nodes_grown, d_prims_grown;  // (a tree over the same objects has up to 2 n - 1 nodes: more than the uploaded one may have had)
  if (ctx->d_scene_nodes.bytes < scene_nodes.size() * 16)
    if (int rc = stage_alloc(ctx, d_nodes_grown, (size_t)(2 * total) * 32)) return rc;
  if (ctx->d_scene_prims.bytes < scene_prims.size() * 4)
    if (int rc = stage_alloc(ctx, d_prims_grown, scene_prims.size() * 4)) return rc;
  const bool general_rows = [&] {  // (the material table's verdict, as the upload and yh_update_materials reach it)
    const bool                mapped = !ctx->h_maps.empty();
    std::vector<yhd_material> rows((size_t)num_materials);
    std::vector<yhd_maps>     dmaps(mapped ? (size_t)num_materials : 0);
    return make_material_rows(ctx->h_materials.data(), mapped ? ctx->h_maps.data() : nullptr, num_materials, rows.data(), dmaps.data());
  }();
  // ---- COMMIT ----
  ctx->have_scene = false;
  if (d_nodes_grown.p) std::swap(ctx->d_scene_nodes.p, d_nodes_grown.p), std::swap(ctx->d_scene_nodes.bytes, d_nodes_grown.bytes);
  if (d_prims_grown.p) std::swap(ctx->d_scene_prims.p, d_prims_grown.p), std::swap(ctx->d_scene_prims.bytes, d_prims_grown.bytes);
  if (count > 0) {
    int e = yhk_object_rows(count, d_rows.p, (const float*)ctx->d_shape_roots.p, (yhd_object*)ctx->d_objects.p + first, (float*)d_boxes.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "object rows: %s", hipGetErrorString((hipError_t)e));
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_nodes.p, scene_nodes.data(), scene_nodes.size() * 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_scene_prims.p, scene_prims.data(), scene_prims.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (scene_wide) {  // the reserved front of the blob: zero as the upload leaves what it does not use, then the new nodes
    HIPCHK(ctx, hipMemsetAsync(ctx->d_lane_blob.p, 0, (size_t)ctx->scene_wide_room * 128, ctx->stream));
    int e = yhk_wide_collapse(2, nn, (const float*)d_stree.p, (const unsigned int*)d_sflag.p, (const unsigned int*)d_sidx.p, 1, 0, 0, ctx->d_lane_blob.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "wide collapse of the scene tree: %s", hipGetErrorString((hipError_t)e));
  }
  YH_WAIT(ctx);
  if (count > 0) memcpy(ctx->key_geometry.data() + sizeof(yh_object) * (size_t)first, objects, sizeof(yh_object) * (size_t)count);
  ctx->h_obj_boxes.swap(boxes);
  ctx->stack_need = needs.need, ctx->stack_need8 = needs.need8, ctx->stack_need16 = needs.need16;
  yhd_scene& sc = ctx->scene;
  sc.scene_nodes = (const yhd_float4*)ctx->d_scene_nodes.p, sc.scene_prims = (const int*)ctx->d_scene_prims.p;
  sc.num_scene_nodes = nn;
  sc.lds_scene_f4    = scene_wide ? 0 : lds_scene_f4;
  sc.scene_wide_root = scene_wide ? 0 : -1;
  sc.stack_entries   = std::max(8, (needs.need + 7) / 8 * 8);
  sc.stack_entries8  = std::max(8, (needs.need8 + 7) / 8 * 8);
  sc.stack_entries16 = std::max(8, (needs.need16 + 7) / 8 * 8);
  settle_scene_variant(ctx, sc, general_rows);
  ctx->have_scene = true;
  edit_end(ctx);
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
