// shape_edit.cpp — edits of ONE shape's vertices in an uploaded scene: yh_update_shape / _device (set_positions / set_normals / set_radius,
// then init_bvh: yocto_pathtrace.h:154-157 — that shape's tree, records and nodes again) and yh_refit_shape / _device (the same edit in
// the tree the shape has: its records and boxes only, unit/refit.hip). No other shape is read, written or moved; the shape's root box
// moves the world boxes of the objects that name it, so the scene level follows as after yh_update_objects (scene_edit.cpp), and an
// emitter's lights get their entries again where they are (light_edit.cpp). The two entry points share passages, not control flow: each
// passage below is a function that QUEUES work on the context's stream and never waits — where an edit waits is the entry point's matter.
// Also what a caller reads of a shape's nodes: yh_shape_nodes, yh_shape_refit_growth.
#include "edit_internal.h"

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
  rows  = uploaded_rows(ctx);
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
      if (int rc = dev_alloc(ctx, buf, bytes)) return rc;
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
  if (int rc = dev_alloc(ctx, A.d_flag, 4)) return rc;
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
  if (int rc = dev_alloc(ctx, d_part, sizeof(double) * (size_t)at.back())) return rc;
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

// ---- the passages yh_update_shape and yh_refit_shape share: each queues its work and returns ----------------------------------------------

// The fingerprint's bytes of the shape: its first and last 256 positions, into key_bytes. positions: the host's array, copied here and
// now, or (device) the device's, fetched by two copies on the stream: key_bytes holds them after the caller's next wait.
static int queue_key_bytes(yh_context* ctx, bool device, const float* positions, size_t nv, std::vector<unsigned char>& key_bytes) {
  const size_t take = std::min<size_t>(nv, 256);
  key_bytes.resize(2 * take * 12);
  if (device) {
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data(), positions, take * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(key_bytes.data() + take * 12, positions + 3 * (nv - take), take * 12, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    memcpy(key_bytes.data(), positions, take * 12), memcpy(key_bytes.data() + take * 12, positions + 3 * (nv - take), take * 12);
  }
  return YH_OK;
}

// The world boxes of the objects that name the shape, from a root box the context does not have yet: their rows name row 0 of a table of
// that one box (the context's table of root boxes changes at COMMIT only). named: their indices; boxes[k]: the world box of object
// named[k], there after the caller's next wait. d_rows holds EVERY object row, d_boxes has room for every object's box: the commit
// below writes the named objects' rows and boxes at their own places.
namespace {
struct NamedBoxes {
  std::vector<int>       named;
  std::vector<yh_object> named_rows;
  std::vector<yhh::Box>  boxes;
  yhh::Box               root{};
  DevBuf                 d_rows, d_boxes, d_named, d_root;
};
}  // namespace
static int queue_named_boxes(yh_context* ctx, const char* who, int shape, const std::vector<yh_object>& rows, const yhh::Box& root, NamedBoxes& N) {
  const size_t total = rows.size();
  for (int i = 0; i < (int)total; i++)
    if (rows[(size_t)i].shape == shape) N.named.push_back(i);
  if (int rc = dev_alloc(ctx, N.d_rows, sizeof(yh_object) * total)) return rc;
  if (int rc = dev_alloc(ctx, N.d_boxes, sizeof(yhh::Box) * total)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(N.d_rows.p, rows.data(), sizeof(yh_object) * total, hipMemcpyHostToDevice, ctx->stream));
  N.root = root;
  N.boxes.resize(N.named.size()), N.named_rows.resize(N.named.size());
  for (size_t k = 0; k < N.named.size(); k++) N.named_rows[k] = rows[(size_t)N.named[k]], N.named_rows[k].shape = 0;
  if (N.named.empty()) return YH_OK;
  if (int rc = dev_alloc(ctx, N.d_named, sizeof(yh_object) * N.named.size())) return rc;
  if (int rc = dev_alloc(ctx, N.d_root, sizeof(yhh::Box))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(N.d_named.p, N.named_rows.data(), sizeof(yh_object) * N.named.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(N.d_root.p, &N.root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
  int e = yhk_object_rows((int)N.named.size(), N.d_named.p, (const float*)N.d_root.p, nullptr, (float*)N.d_boxes.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
  HIPCHK(ctx, hipMemcpyAsync(N.boxes.data(), N.d_boxes.p, sizeof(yhh::Box) * N.named.size(), hipMemcpyDeviceToHost, ctx->stream));
  return YH_OK;
}

// ... and, at COMMIT, the rows of those objects in the context's table, from its table of root boxes (the shape's new one queued before):
// run by run of consecutive ones, so that no other object's row is written
static int commit_named_rows(yh_context* ctx, const char* who, const NamedBoxes& N) {
  const std::vector<int>& named = N.named;
  int e = 0;
  for (size_t k = 0; k < named.size() && !e;) {
    size_t end_k = k + 1;
    while (end_k < named.size() && named[end_k] == named[end_k - 1] + 1) end_k++;
    const int first = named[k], run = (int)(end_k - k);
    e = yhk_object_rows(run, (const yh_object*)N.d_rows.p + first, (const float*)ctx->d_shape_roots.p, (yhd_object*)ctx->d_objects.p + first, (float*)N.d_boxes.p + 6 * (size_t)first, ctx->stream);
    k = end_k;
  }
  if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

// The shape's rows of the per-vertex arrays (a shape that has some), from its arrays on the device
static int queue_vertex_rows(yh_context* ctx, const char* who, const yh_context::ShapeState& E, const yh_shape& dev, bool lines, size_t nel) {
  if (!E.per_vertex) return YH_OK;
  int e = yhk_vertex_rows(lines ? 1 : 0, dev.num_vertices, (int)nel, dev.positions, dev.radius, dev.texcoords, lines ? dev.lines : dev.triangles,
      (yhd_float4*)ctx->d_vpos.p + E.vert_base, (float*)ctx->d_vtex.p + 2 * (size_t)E.vert_base, (yhd_int4*)ctx->d_elems.p + E.elem_base, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%svertex rows: %s", who, hipGetErrorString((hipError_t)e));
  return YH_OK;
}

// ---- yh_update_shape / yh_update_shape_device -----------------------------------------------------------------------------------------------
// One shape's leaf records, test records, 4- / 8- / 16-wide nodes and per-vertex rows are made again with the upload's own code
// (scene_upload.cpp: build_shape_tree, index_shape_tree, collapse_shape_tree) and unit/shapes.hip. The node counts depend on the
// positions: a width whose new count exceeds the room of the shape's region gets a new region behind the end of the traversal array
// (count + count / 8 nodes, on a multiple of 4 units), the array is reallocated and the old bytes copied device to device, the vacated
// region is zeroed and stays unused until an upload (the rule: blob_layout.h). No other shape moves: the collapse writes absolute references.
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
  const yh_shape& dev = A.dev;
  // ---- the tree, the records and the index of the wide nodes: the upload's rule for where, the upload's code ----
  const bool on_device = device || shape_builds_on_device((int)nel);
  ShapeTree  T;
  DevBuf     d_recs;
  if (int rc = dev_alloc(ctx, d_recs, nel * per * 16)) return rc;
  if (int rc = build_shape_tree(ctx, who, shape, on_device ? dev : *now, on_device, on_device, (yhd_float4*)d_recs.p, T)) return rc;
  if (int rc = index_shape_tree(ctx, who, T)) return rc;
  // ---- where the wide nodes go (blob_layout.h: blob_growth) ----
  const long long old_units = ctx->scene.lane_blob_units, old_off[3] = {L.node_off, L.node_off8, L.node_off16};
  BlobGrowth      G;
  if (blob_growth(old_units, old_off, E.room, T.wide_count, G) != YH_BLOB_OK)
    return fail(ctx, YH_E_INVALID, "%sscene too large for 30-bit node offsets (%lld units): upload the scene", who, G.units);
  const long long       end  = G.units;
  yh_context::LaneShape Lnew = L;
  Lnew.num_nodes = T.wide_count[0], Lnew.node_off = G.off[0], Lnew.node_off8 = G.off[1], Lnew.node_off16 = G.off[2];
  DevBuf d_blob_grown;
  if (end > old_units)
    if (int rc = dev_alloc(ctx, d_blob_grown, (size_t)end * 32)) return rc;
  const ShapeDepths deepest = deepest_shape_trees(ctx->shape_states, shape, &T);
  // ---- the world boxes of the objects that name the shape, from its new root box; the scene level over all boxes ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  NamedBoxes            N;
  if (int rc = queue_named_boxes(ctx, who, shape, rows, T.root, N)) return rc;
  std::vector<unsigned char> key_bytes;
  if (int rc = queue_key_bytes(ctx, device, now->positions, nv, key_bytes)) return rc;
  YH_WAIT(ctx);
  for (size_t k = 0; k < N.named.size(); k++) boxes[(size_t)N.named[k]] = N.boxes[k];
  SceneLevelStage S;
  if (int rc = stage_scene_level(ctx, entry, boxes, deepest.depth4, deepest.depth8, deepest.depth16, S)) return rc;
  LightStage LS;  // an emitter's shape: the cdf and the record of the lights that name it, made once the new arrays sit in the context's rows
  if (emits)
    if (int rc = stage_lights_of_shape(ctx, shape, rows.data(), LS)) return rc;
  // ---- COMMIT: from here on kernels, copies and memsets only ----
  ctx->have_scene = false;
  if (d_blob_grown.p) {  // the old array's bytes as they are, zeros behind them (what alloc_zero leaves)
    HIPCHK(ctx, hipMemcpyAsync(d_blob_grown.p, ctx->d_lane_blob.p, (size_t)old_units * 32, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync((char*)d_blob_grown.p + (size_t)old_units * 32, 0, (size_t)(end - old_units) * 32, ctx->stream));
    ctx->d_lane_blob.swap(d_blob_grown);
    ctx->scene.lane_blob = nullptr;
  }
  for (int w = 0; w < 3; w++)  // the shape's regions as they were: vacated, or written again with the unused rest zero
    if (E.room[w] > 0) HIPCHK(ctx, hipMemsetAsync((char*)ctx->d_lane_blob.p + (size_t)old_off[w] * 32, 0, (size_t)YH_BLOB_WIDTH[w] * E.room[w] * 32, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync((yhd_float4*)ctx->d_prims.p + L.prim_base, d_recs.p, nel * per * 16, hipMemcpyDeviceToDevice, ctx->stream));
  if (int rc = collapse_shape_tree(ctx, who, T, Lnew, ctx->d_lane_blob.p)) return rc;
  if (int rc = queue_vertex_rows(ctx, who, E, dev, lines, nel)) return rc;
  HIPCHK(ctx, hipMemcpyAsync((yhh::Box*)ctx->d_shape_roots.p + shape, &T.root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = commit_named_rows(ctx, who, N)) return rc;
  {  // ... then the lane roots: the shape's nodes may have moved
    int e = yhk_object_lane_roots(total, N.d_rows.p, shape, (int)Lnew.node_off, (int)Lnew.node_off8, (int)Lnew.node_off16, ctx->d_objects.p, ctx->stream);
    if (e) return fail(ctx, YH_E_DEVICE, "%sobject rows: %s", who, hipGetErrorString((hipError_t)e));
  }
  if (int rc = commit_scene_level(ctx, S)) return rc;
  if (emits)
    if (int rc = commit_lights_of_shape(ctx, entry, LS)) return rc;
  YH_WAIT(ctx);
  memcpy(ctx->key_geometry.data() + E.key_positions, key_bytes.data(), key_bytes.size());
  ctx->scene.num_nodes_total += T.wide_count[0] - E.count[0];
  double area[3];
  if (int rc = shape_slot_areas(ctx, who, 1, &Lnew, &T.wide_count, ctx->d_lane_blob.p, area)) return rc;
  ctx->lane_shapes[(size_t)shape] = Lnew;
  shape_state_of_build(ctx->shape_states[(size_t)shape], T, G.room, area);  // (E and L are these: not read below)
  ctx->lane_units = 0;
  for (int s = 0; s < num_shapes; s++)  // the end of the furthest 4-wide region: what the one-lane kernels address
    ctx->lane_units = std::max(ctx->lane_units, blob_lane_end(ctx->lane_shapes[(size_t)s].node_off, ctx->shape_states[(size_t)s].room[0]));
  ctx->scene.lane_blob = (const yhd_float4*)ctx->d_lane_blob.p, ctx->scene.lane_blob_units = end;
  ctx->h_shape_roots[(size_t)shape] = T.root;
  ctx->h_obj_boxes.swap(boxes);
  ctx->max_shape_depth = deepest.depth4, ctx->max_shape_depth8 = deepest.depth8, ctx->max_shape_depth16 = deepest.depth16;
  settle_scene_level(ctx, S);
  ctx->have_scene = true;
  for (size_t o = 0; o < rows.size(); o++)  // (the shape's objects: their pixels of the temporal history are not reused)
    if (rows[o].shape == shape) temporal_mark_object(ctx, (int)o);
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
  if (int rc = dev_alloc(ctx, d_lboxes, nel * sizeof(yhh::Box))) return rc;
  if (int rc = dev_alloc(ctx, d_part, sizeof(yhh::Box) * (size_t)parts)) return rc;
  int e = yhk_refit_boxes(lines ? 1 : 0, (int)nel, d_recs, dev.positions, dev.radius, d_index, (float*)d_lboxes.p, ctx->stream);
  if (!e) e = yhk_box_partials((int)nel, (const float*)d_lboxes.p, (float*)d_part.p, ctx->stream);
  if (e) return fail(ctx, YH_E_DEVICE, "%sprimitive bounds: %s", who, hipGetErrorString((hipError_t)e));
  std::vector<yhh::Box> part((size_t)parts);
  HIPCHK(ctx, hipMemcpyAsync(part.data(), d_part.p, sizeof(yhh::Box) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  std::vector<unsigned char> key_bytes;
  if (int rc = queue_key_bytes(ctx, device, now->positions, nv, key_bytes)) return rc;
  YH_WAIT(ctx);
  yhh::Box root = part[0];
  for (int k = 1; k < parts; k++)
    for (int c = 0; c < 3; c++) root.min[c] = fmin_(root.min[c], part[(size_t)k].min[c]), root.max[c] = fmax_(root.max[c], part[(size_t)k].max[c]);
  // ---- the world boxes of the objects that name the shape, from its new root box; the scene level over all boxes ----
  std::vector<yhh::Box> boxes = ctx->h_obj_boxes;
  NamedBoxes            N;
  if (int rc = queue_named_boxes(ctx, who, shape, rows, root, N)) return rc;
  if (!N.named.empty()) YH_WAIT(ctx);
  for (size_t k = 0; k < N.named.size(); k++) boxes[(size_t)N.named[k]] = N.boxes[k];
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
  if (int rc = queue_vertex_rows(ctx, who, E, dev, lines, nel)) return rc;
  HIPCHK(ctx, hipMemcpyAsync((yhh::Box*)ctx->d_shape_roots.p + shape, &root, sizeof(yhh::Box), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = commit_named_rows(ctx, who, N)) return rc;  // (their lane roots stay: nothing moved)
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
  for (size_t o = 0; o < rows.size(); o++)  // (the shape's objects: their pixels of the temporal history are not reused)
    if (rows[o].shape == shape) temporal_mark_object(ctx, (int)o);
  edit_end(ctx);
  return YH_OK;
}

int yh_refit_shape(yh_context* ctx, int shape, const yh_shape* now) { return refit_shape(ctx, "yh_refit_shape", shape, now, false); }
int yh_refit_shape_device(yh_context* ctx, int shape, const yh_shape* now) { return refit_shape(ctx, "yh_refit_shape_device", shape, now, true); }

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
