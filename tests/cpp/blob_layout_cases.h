// The inputs of tests/cpp/test_blob_layout.cpp, apart from the program so that whatever writes tests/golden/blob_layout.txt reads the
// same table. Counts only: nothing here is laid out.
#ifndef YH_BLOB_LAYOUT_CASES_H_
#define YH_BLOB_LAYOUT_CASES_H_
#include <stdio.h>

#include <string>
#include <vector>

struct CaseShape {
  bool lines;
  int  num_prims, count[3];
};
struct LayoutCase {
  const char*            name;
  bool                   scene_wide;
  int                    num_objects;
  std::vector<CaseShape> shapes;
  int                    expect;  // 0 fits, 1 the 27-bit refusal, 2 the 30-bit one
};
static const std::vector<LayoutCase> layout_cases = {
    {"one_line_shape", false, 1, {{true, 1000, {333, 143, 67}}}, 0},
    {"one_triangle_shape", false, 1, {{false, 12, {3, 1, 1}}}, 0},
    {"lines_and_triangles", false, 3, {{true, 1601, {533, 229, 107}}, {false, 7, {2, 1, 1}}, {true, 5, {1, 1, 1}}}, 0},
    {"no_16_wide_nodes", false, 2, {{false, 2, {1, 1, 0}}, {true, 9, {3, 1, 0}}}, 0},
    {"scene_level_wide", true, 100, {{true, 1601, {533, 229, 107}}, {false, 7, {2, 1, 1}}}, 0},
    {"scene_level_not_wide", false, 100, {{true, 1601, {533, 229, 107}}, {false, 7, {2, 1, 1}}}, 0},
    {"scene_level_wide_odd_objects", true, 47, {{false, 1, {1, 1, 1}}}, 0},
    {"counts_not_multiples_of_four", false, 3, {{true, 3, {1, 1, 1}}, {false, 1, {1, 1, 1}}, {true, 10, {3, 2, 1}}}, 0},
    // the test records end at align4(n) + 4 units: 2^27 - 4 passes, 2^27 is refused
    {"leaf_offsets_just_under", false, 1, {{true, (1 << 27) - 8, {1, 1, 1}}}, 0},
    {"leaf_offsets_at_limit", false, 1, {{true, (1 << 27) - 7, {1, 1, 1}}}, 1},
    // 1 record -> 8; two 4-wide nodes -> 16, lane_units 20; one 8-wide -> 28; c 16-wide -> 28 + 16 c; + 4 = 32 + 16 c
    {"node_offsets_just_under", false, 1, {{true, 1, {2, 1, (1 << 26) - 3}}}, 0},
    {"node_offsets_at_limit", false, 1, {{true, 1, {2, 1, (1 << 26) - 2}}}, 2},
};

struct GrowthCase {
  const char* name;
  long long   old_units, old_off[3];
  int         old_room[3], count[3];
  int         expect;  // 0 fits, 2 the 30-bit refusal
};
static const std::vector<GrowthCase> growth_cases = {
    {"every_width_fits", 1000, {100, 200, 400}, {10, 5, 3}, {10, 4, 3}, 0},
    {"four_wide_grows", 1000, {100, 200, 400}, {10, 5, 3}, {11, 5, 3}, 0},
    {"eight_and_sixteen_grow_from_an_unaligned_end", 1053, {100, 200, 400}, {10, 5, 3}, {10, 9, 17}, 0},
    {"every_width_grows", 2048, {100, 200, 400}, {10, 5, 3}, {100, 50, 30}, 0},
    {"counts_below_eight_get_no_spare", 512, {100, 200, 400}, {1, 1, 1}, {7, 7, 7}, 0},
    // 16-wide: room 9 (8 + 8 / 8) -> 144 units + 4 behind old_units
    {"growth_just_under_the_limit", (1ll << 30) - 152, {100, 200, 400}, {10, 5, 3}, {10, 5, 8}, 0},
    {"growth_at_the_limit", (1ll << 30) - 148, {100, 200, 400}, {10, 5, 3}, {10, 5, 8}, 2},
};

// one line of tests/golden/blob_layout.txt per case; after a refusal only the code and the figure it names
struct RegionLine {
  long long test_off, node_off[3];
};
inline std::string layout_line(const char* name, int rc, long long refused_at, long long lane_units, long long units, const std::vector<RegionLine>& regions) {
  char buf[256];
  if (rc) return snprintf(buf, sizeof(buf), "layout %s rc=%d at=%lld", name, rc, refused_at), std::string(buf);
  snprintf(buf, sizeof(buf), "layout %s rc=0 lane_units=%lld units=%lld regions=", name, lane_units, units);
  std::string line = buf;
  for (const RegionLine& r : regions) snprintf(buf, sizeof(buf), " %lld:%lld:%lld:%lld", r.test_off, r.node_off[0], r.node_off[1], r.node_off[2]), line += buf;
  return line;
}
inline std::string growth_line(const char* name, int rc, long long units, const long long off[3], const int room[3]) {
  char buf[256];
  if (rc) return snprintf(buf, sizeof(buf), "growth %s rc=%d units=%lld", name, rc, units), std::string(buf);
  return snprintf(buf, sizeof(buf), "growth %s rc=0 units=%lld off=%lld,%lld,%lld room=%d,%d,%d", name, units, off[0], off[1], off[2], room[0], room[1], room[2]), std::string(buf);
}
#endif
