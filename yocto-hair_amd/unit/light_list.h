// light_list.h — what unit/light_list.hip and the host's share of a light edit (host/scene_edit.cpp) agree on: one job per area light
// of the new list, copied to the device as it is.
#ifndef YH_LIGHT_LIST_H_
#define YH_LIGHT_LIST_H_

typedef struct yhk_light_job {
  int elem_base, vert_base;  // the shape's first row of yhd_scene::elems / vpos
  int count;                 // its triangles: the light's cdf entries
  int cdf_base;              // where they go in the new light_cdf
  int prim_base, shape;      // a small light's record: the shape's first leaf record (float4 units), its row of the root boxes
  int small_base;            // ... and its float4 in the new light table, -1: a light read through memory
  int pad;
} yhk_light_job;

#endif
