// edit_internal.h — what crosses the files that make and edit an uploaded scene (scene_upload.cpp, scene_edit.cpp, shape_edit.cpp,
// light_edit.cpp): how an edit begins and ends, the description the context keeps, the rules the upload and the edits both follow — the
// scene level (scene_upload.cpp: derive_scene_level), a shape's state from a build, the light fields of the scene table; the layouts are
// light_layout.h's and blob_layout.h's — and the two stagings more than one edit runs: the scene level again (scene_edit.cpp) and the
// light list again (light_edit.cpp). Every stage_* computes and allocates what can refuse and writes nothing the kernels read; every
// commit_* queues kernels, copies and memsets on the context's stream and never waits. Not installed.
#ifndef YH_EDIT_INTERNAL_H_
#define YH_EDIT_INTERNAL_H_
#include "context_internal.h"
#include "blob_layout.h"
#include "light_layout.h"  // LightLayout, is_black
#include "upload_stages.h"  // append_env_cdf

#pragma GCC visibility push(hidden)  // internal to libyhair.so
// ---- scene_edit.cpp ----
// what every edit starts with: a context that can take it (an uploaded scene, no launch in flight) ... and ends with: the fingerprint of
// the edited description, no image state, nothing planned
int  edit_begin(yh_context* ctx, const char* entry);
void edit_end(yh_context* ctx);
// every object row as it was passed in, the environments' emission in force (3 floats each, YH_MAX_ENVS of them), and the material
// table's verdict as the upload and yh_update_materials reach it
std::vector<yh_object> uploaded_rows(const yh_context* ctx);
std::vector<float>     emission_in_force(const yh_context* ctx);
bool                   general_rows_in_force(const yh_context* ctx);

// The scene level. derive_scene_level (scene_upload.cpp) is the rule, for the upload and for every edit that moves a world box: the
// reference's tree over `boxes` (every object's world box), whether it is walked as 4-wide nodes (then their index on the device), the
// stack needs (depth4 / 8 / 16: the deepest shape tree as 4- / 8- / 16-wide nodes; check_stack_needs: the check every scene has to pass),
// the node pairs and the padded primitive list. collapse_scene_tree queues the wide nodes into a traversal array; set_scene_level_fields
// brings the scene table and the three stack sizes in line. `who` begins every message ("" for the upload, "<entry>: " for an edit).
// The scene level AGAIN: stage_scene_level derives it and adds what is an edit's own — the refusals (wide / not wide as uploaded, the room
// the upload left), grown buffers, the material table's verdict; commit_scene_level queues the copies, the memset and the collapse;
// settle_scene_level, once they are done, brings the host's side of the scene table in line.
struct SceneLevelStage {
  yhh::Tree  tree;
  int        nn = 0, lds_scene_f4 = 0, wide_count = 0, wide_depth = 0;
  bool       scene_wide = false, general_rows = false;
  DevBuf     d_stree, d_sflag, d_sidx, d_nodes_grown, d_prims_grown;
  StackNeeds needs{};
  std::vector<yhd_float4> scene_nodes;
  std::vector<int>        scene_prims;
};
int  derive_scene_level(yh_context* ctx, const char* who, const std::vector<yhh::Box>& boxes, int num_objects, int depth4, int depth8, int depth16, SceneLevelStage& S);
int  check_stack_needs(yh_context* ctx, const char* who, const StackNeeds& needs);
int  collapse_scene_tree(yh_context* ctx, const SceneLevelStage& S, void* blob);
void set_scene_level_fields(yh_context* ctx, yhd_scene& sc, const SceneLevelStage& S);
int  stage_scene_level(yh_context* ctx, const char* entry, const std::vector<yhh::Box>& boxes, int depth4, int depth8, int depth16, SceneLevelStage& S);
int  commit_scene_level(yh_context* ctx, SceneLevelStage& S);
void settle_scene_level(yh_context* ctx, const SceneLevelStage& S);

// scene_upload.cpp: what a built shape leaves in its ShapeState — depths, counts, `room` per width, the levels of its wide trees, `area`
// as built and now
void shape_state_of_build(yh_context::ShapeState& E, const ShapeTree& T, const int room[3], const double area[3]);

// ---- light_edit.cpp ----
// the light fields of a scene table whose light arrays are in the context's buffers (the upload, commit_lights)
void set_light_fields(yh_context* ctx, yhd_scene& sc, const LightLayout& L);
// The light list again (yh_set_light_edits). stage_lights lays the list out over the description as the edit leaves it (materials: the
// whole table; rows: every object row; emission: 3 floats per environment) and allocates the new arrays; commit_lights fills them and
// swaps them in: the old arrays go when the stage does, after the caller's wait. A VERTEX edit of an emitter's shape moves no light:
// stage_lights_of_shape / commit_lights_of_shape write the entries of that shape's lights where they are.
struct LightStage {
  LightLayout layout;
  std::vector<yhk_light_job> jobs;  // the area lights, in list order
  DevBuf      d_jobs, d_cdf, d_table, d_tab;
};
int stage_lights(yh_context* ctx, const char* entry, const yh_material* materials, const yh_object* rows, const float* emission, LightStage& S);
int commit_lights(yh_context* ctx, const char* entry, LightStage& S);
int stage_lights_of_shape(yh_context* ctx, int shape, const yh_object* rows, LightStage& S);
int commit_lights_of_shape(yh_context* ctx, const char* entry, LightStage& S);
#pragma GCC visibility pop
#endif
