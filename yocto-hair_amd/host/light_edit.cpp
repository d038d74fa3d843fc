// light_edit.cpp — the light list of an uploaded scene, made again by the edits that change it (yh_set_light_edits, off by default: without
// it they refuse). The rule is the upload's (light_layout.h); the area cdfs, the small lights' records and the coarse index of a texel cdf
// are made on the device (unit/light_list.hip) from the rows the context keeps there, where the upload computes them on the host from
// the arrays it was lent. Also what a caller reads of the list (yh_light_list) and the area cdf of one shape in both forms
// (yh_triangle_cdf / _gpu).
#include "edit_internal.h"

// stage_lights refuses what the upload refuses (more than YH_MAX_LIGHTS lights, none at all), allocates the new light_cdf and light table
// and sees to it that every textured environment of the new list has its texel cdf on the device (ctx->d_env_cdf: saved from the
// light_cdf in force, or made with the upload's loop from the texels read back from d_env_texels — the host's sine, upload_stages.h:
// append_env_cdf). Nothing the kernels read is written.
int stage_lights(yh_context* ctx, const char* entry, const yh_material* materials, const yh_object* rows, const float* emission, LightStage& S) {
  const yhd_scene& sc = ctx->scene;
  LightLayout&     L  = S.layout;
  std::vector<LightShape> shapes;
  for (const yh_context::LaneShape& ls : ctx->lane_shapes) shapes.push_back({ls.kind == YH_KIND_LINES, ls.num_prims});
  int texels[YH_MAX_ENVS] = {};
  for (int ei = 0; ei < sc.num_environments; ei++) texels[ei] = sc.environments[ei].tex_w * sc.environments[ei].tex_h;
  int at = 0;
  switch (light_layout({sc.num_objects, rows, materials, shapes.data(), sc.num_environments, emission, texels}, L, &at)) {
    case YH_LIGHTS_OBJECT_TOO_MANY:
      return fail(ctx, YH_E_INVALID, "%s: more than %d lights: object %d of %d is emissive too (each instance of an emitter counts)", entry, YH_MAX_LIGHTS, at, sc.num_objects);
    case YH_LIGHTS_ENVIRONMENT_TOO_MANY: return fail(ctx, YH_E_INVALID, "%s: more than %d lights: environment %d is one too", entry, YH_MAX_LIGHTS, at);
    case YH_LIGHTS_NONE:
      return fail(ctx, YH_E_INVALID, "%s: the edit leaves the scene without a light (the path sampler needs at least one): upload the scene", entry);
  }
  if (L.cdf_total > (size_t)std::numeric_limits<int>::max()) return fail(ctx, YH_E_INVALID, "%s: light cdf of %zu entries", entry, L.cdf_total);
  for (int li = 0; li < L.num_lights; li++) {
    const yhd_light& l = L.lights[li];
    if (l.object < 0) continue;
    const int shape = rows[l.object].shape;
    const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
    S.jobs.push_back({E.elem_base, E.vert_base, l.cdf_count, l.cdf_base, ctx->lane_shapes[(size_t)shape].prim_base, shape, l.small_base, 0});
  }
  // the texel cdf of every textured environment that is a light now or will be one: kept on the device from here on. (A cache that no
  // entry point shows and whose content depends on the texels alone: a call refused further down leaves it filled, and is still
  // "the context exactly as it was" for everything a caller can observe.)
  auto kept = [&](int ei, int count, const float* d_segment) -> int {
    DevBuf& buf = ctx->d_env_cdf[ei];
    if (buf.p || count <= 0) return YH_OK;
    DevBuf made;
    if (int rc = dev_alloc(ctx, made, (size_t)count * 4)) return rc;
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
    buf.swap(made);
    return YH_OK;
  };
  for (int li = 0; li < sc.num_lights; li++)
    if (sc.lights[li].environment >= 0)
      if (int rc = kept(sc.lights[li].environment, sc.lights[li].cdf_count, (const float*)ctx->d_light_cdf.p + sc.lights[li].cdf_base)) return rc;
  for (int li = 0; li < L.num_lights; li++)
    if (L.lights[li].environment >= 0)
      if (int rc = kept(L.lights[li].environment, L.lights[li].cdf_count, nullptr)) return rc;
  if (int rc = dev_alloc(ctx, S.d_cdf, L.cdf_total * 4)) return rc;
  if (int rc = dev_alloc(ctx, S.d_table, (size_t)L.table_f4 * 16)) return rc;
  if (int rc = dev_alloc(ctx, S.d_tab, (size_t)L.env_tab_k * 4)) return rc;
  if (int rc = dev_alloc(ctx, S.d_jobs, S.jobs.size() * sizeof(yhk_light_job))) return rc;
  return YH_OK;
}

// queues the kernels and copies into the NEW arrays on the context's stream and brings the scene table in line
int commit_lights(yh_context* ctx, const char* entry, LightStage& S) {
  const LightLayout& L  = S.layout;
  const int          nj = (int)S.jobs.size();
  if (nj > 0) HIPCHK(ctx, hipMemcpyAsync(S.d_jobs.p, S.jobs.data(), S.jobs.size() * sizeof(yhk_light_job), hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_light_cdfs(nj, S.d_jobs.p, ctx->d_vpos.p, ctx->d_elems.p, (float*)S.d_cdf.p, ctx->stream);
  if (!e) e = yhk_small_records(nj, S.d_jobs.p, (const float*)ctx->d_shape_roots.p, ctx->d_prims.p, (const float*)S.d_cdf.p, S.d_table.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: light list: %s", entry, hipGetErrorString((hipError_t)e));
  for (int li = 0; li < L.num_lights; li++) {  // an environment light's segment: a copy of the cdf the context keeps
    const yhd_light& l = L.lights[li];
    if (l.environment >= 0 && l.cdf_count > 0)
      HIPCHK(ctx, hipMemcpyAsync((float*)S.d_cdf.p + l.cdf_base, ctx->d_env_cdf[l.environment].p, (size_t)l.cdf_count * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  if (L.env_tab_light >= 0) {
    const yhd_light& l = L.lights[L.env_tab_light];
    e = yhk_env_tab(L.env_tab_k, L.env_tab_stride, l.cdf_count, (const float*)S.d_cdf.p + l.cdf_base, (float*)S.d_tab.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%s: coarse index of the environment cdf: %s", entry, hipGetErrorString((hipError_t)e));
  }
  ctx->d_light_cdf.swap(S.d_cdf), ctx->d_light_table.swap(S.d_table), ctx->d_env_tab.swap(S.d_tab);
  temporal_drop(ctx);  // (another light list: the temporal history shows another lighting)
  set_light_fields(ctx, ctx->scene, L);  // (settle_scene_variant reads them: the caller runs that next)
  return YH_OK;
}

void set_light_fields(yh_context* ctx, yhd_scene& sc, const LightLayout& L) {
  sc.num_lights = L.num_lights;
  memcpy(sc.lights, L.lights, sizeof(sc.lights));
  sc.light_cdf = (const float*)ctx->d_light_cdf.p;
  sc.light_table = (const yhd_float4*)ctx->d_light_table.p, sc.light_table_f4 = L.table_f4;
  sc.env_tab = (const float*)ctx->d_env_tab.p;
  sc.env_tab_light = L.env_tab_light, sc.env_tab_k = L.env_tab_k, sc.env_tab_stride = L.env_tab_stride;
  ctx->big_lights = L.big_lights;  // (a light sampled and intersected through memory: the general kernel variant)
}

// A VERTEX edit of an emitter's shape changes no light's place: the list, every offset, the kernel variant and every other light's
// entries stay. Only the lights that name `shape` get their cdf segment and their small record again, written where they are, from the
// rows, records and root box the edit has queued on the stream before. rows: every object row.
int stage_lights_of_shape(yh_context* ctx, int shape, const yh_object* rows, LightStage& S) {
  const yhd_scene& sc = ctx->scene;
  for (int li = 0; li < sc.num_lights; li++) {
    const yhd_light& l = sc.lights[li];
    if (l.object < 0 || rows[l.object].shape != shape) continue;
    const yh_context::LaneShape&  L = ctx->lane_shapes[(size_t)shape];
    const yh_context::ShapeState& E = ctx->shape_states[(size_t)shape];
    S.jobs.push_back({E.elem_base, E.vert_base, l.cdf_count, l.cdf_base, L.prim_base, shape, l.small_base, 0});
  }
  return dev_alloc(ctx, S.d_jobs, S.jobs.size() * sizeof(yhk_light_job));
}
int commit_lights_of_shape(yh_context* ctx, const char* entry, LightStage& S) {
  const int nj = (int)S.jobs.size();
  if (nj == 0) return YH_OK;
  HIPCHK(ctx, hipMemcpyAsync(S.d_jobs.p, S.jobs.data(), S.jobs.size() * sizeof(yhk_light_job), hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_light_cdfs(nj, S.d_jobs.p, ctx->d_vpos.p, ctx->d_elems.p, (float*)ctx->d_light_cdf.p, ctx->stream);
  if (!e) e = yhk_small_records(nj, S.d_jobs.p, (const float*)ctx->d_shape_roots.p, ctx->d_prims.p, (const float*)ctx->d_light_cdf.p, ctx->d_light_table.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%s: light list: %s", entry, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

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
  if (ctx->poisoned) return refuse_poisoned(ctx);
  YH_WAIT(ctx);
  const yhk_light_job job{0, 0, num_triangles, 0, 0, 0, -1, 0};
  DevBuf d_job, d_pos, d_tri, d_cdf;
  if (int rc = dev_alloc(ctx, d_job, sizeof(job))) return rc;
  if (int rc = dev_alloc(ctx, d_pos, (size_t)num_vertices * 12)) return rc;
  if (int rc = dev_alloc(ctx, d_tri, (size_t)num_triangles * 12)) return rc;
  if (int rc = dev_alloc(ctx, d_cdf, (size_t)num_triangles * 4)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(d_job.p, &job, sizeof(job), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_pos.p, positions, (size_t)num_vertices * 12, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_tri.p, triangles, (size_t)num_triangles * 12, hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_triangle_cdf_raw(d_job.p, (const float*)d_pos.p, (const int*)d_tri.p, (float*)d_cdf.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "yh_triangle_cdf_gpu: %s", hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(cdf, d_cdf.p, (size_t)num_triangles * 4, hipMemcpyDeviceToHost, ctx->stream));
  YH_WAIT(ctx);
  return YH_OK;
}
