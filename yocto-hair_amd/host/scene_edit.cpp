// scene_edit.cpp — edits of an uploaded scene that leave every acceleration structure as it is: the camera, rows of the material table, the
// environments' frames and emission. The reference reads its scene structs live (an interactive caller edits app->camera->frame and traces
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
