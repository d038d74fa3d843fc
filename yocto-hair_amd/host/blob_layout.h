// blob_layout.h — where everything sits in the ONE array the traversal kernels read (yh_device.h: lane_blob, 32-byte units), stated once:
//   [4-wide nodes of the scene tree, if it is walked from here][test records of every shape][4-wide nodes][8-wide nodes][16-wide nodes]
// blob_layout is the whole array as yh_upload_scene makes it (scene_upload.cpp); blob_growth is the step yh_update_shape makes for ONE
// shape whose node counts changed (shape_edit.cpp). Every shape edit is tested bit for bit against a fresh upload, so the two must agree
// on alignment and slack. No HIP call, no context: plain C++ over counts.
#ifndef YH_BLOB_LAYOUT_H_
#define YH_BLOB_LAYOUT_H_
#include <vector>

#pragma GCC visibility push(hidden)  // internal to libyhair.so
struct BlobShape {
  bool lines;      // one test record per segment, two per triangle
  int  num_prims;
  int  count[3];   // its 4- / 8- / 16-wide nodes
};
struct BlobRegions {
  long long test_off, node_off[3];  // the shape's test records and its nodes of each width
};
struct BlobLayout {
  std::vector<BlobRegions> shapes;
  long long lane_units = 0;  // the end of the 4-wide regions: what the one-lane kernels address (32-bit byte offsets: launch_plan.cpp: lane_kernels_can_address)
  long long units = 0;       // the whole array
};
// (*at: the figure the refusal names — the test-record units, the array's units)
enum { YH_BLOB_OK = 0, YH_BLOB_LEAF_OFFSETS, YH_BLOB_NODE_OFFSETS };

constexpr long long YH_BLOB_SLACK      = 4;          // units behind the last test record and the last node of a width: a leaf step reads 64 bytes
constexpr long long YH_BLOB_LEAF_LIMIT = 1ll << 27;  // a leaf reference packs its first record into 27 bits; a scene node's offset stays below it too
constexpr long long YH_BLOB_NODE_LIMIT = 1ll << 30;
constexpr int       YH_BLOB_WIDTH[3]   = {4, 8, 16};  // units per node

inline long long blob_align(long long at) { return (at + 3) / 4 * 4; }  // nodes on 128-byte lines

// The end of a 4-wide region with room for room0 nodes, slack included; lane_units is the furthest of them.
inline long long blob_lane_end(long long node_off, int room0) { return node_off + 4ll * room0 + YH_BLOB_SLACK; }

// scene_wide: the scene level is walked as 4-wide nodes from the front of the array — in front of the test records: a scene node's offset
// stays below 2^27, what tells it from a scene leaf on a stack. Room for as many nodes as the scene has objects: a wide node stands for an
// internal binary node, of which a tree over n objects has at most n - 1, so yh_update_objects can write the nodes of any tree over them;
// the slots behind the ones in use stay zero.
inline int blob_layout(bool scene_wide, int num_objects, const BlobShape* shapes, int num_shapes, BlobLayout& out, long long* at_out) {
  out = BlobLayout{};
  out.shapes.resize((size_t)num_shapes);
  long long at = scene_wide ? 4ll * num_objects : 0;
  for (int si = 0; si < num_shapes; si++) out.shapes[(size_t)si].test_off = at, at += (long long)shapes[si].num_prims * (shapes[si].lines ? 1 : 2);
  at = blob_align(at) + YH_BLOB_SLACK;
  if (at >= YH_BLOB_LEAF_LIMIT) return *at_out = at, YH_BLOB_LEAF_OFFSETS;
  for (int w = 0; w < 3; w++) {
    for (int si = 0; si < num_shapes; si++) out.shapes[(size_t)si].node_off[w] = at, at += (long long)YH_BLOB_WIDTH[w] * shapes[si].count[w];
    if (w == 0) out.lane_units = at + YH_BLOB_SLACK, at = blob_align(out.lane_units);
  }
  out.units = at + YH_BLOB_SLACK;
  if (out.units >= YH_BLOB_NODE_LIMIT) return *at_out = out.units, YH_BLOB_NODE_OFFSETS;
  return YH_BLOB_OK;
}

// One shape built again in an array of old_units: a width whose new count fits the room of its region stays where it is; one that does
// not gets a new region behind the end, aligned, with room for count + count / 8 nodes and the slack behind it. Nothing else moves.
struct BlobGrowth {
  long long off[3];
  int       room[3];
  long long units;  // the array's new end (old_units: it does not grow)
};
inline int blob_growth(long long old_units, const long long old_off[3], const int old_room[3], const int count[3], BlobGrowth& out) {
  out.units = old_units;
  for (int w = 0; w < 3; w++) {
    out.off[w] = old_off[w], out.room[w] = old_room[w];
    if (count[w] <= old_room[w]) continue;
    out.off[w]  = blob_align(out.units);
    out.room[w] = count[w] + count[w] / 8;
    out.units   = out.off[w] + (long long)YH_BLOB_WIDTH[w] * out.room[w] + YH_BLOB_SLACK;
  }
  return out.units >= YH_BLOB_NODE_LIMIT ? YH_BLOB_NODE_OFFSETS : YH_BLOB_OK;
}
#pragma GCC visibility pop
#endif
