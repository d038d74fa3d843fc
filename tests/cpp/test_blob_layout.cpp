// Where everything sits in the traversal array (yocto-hair_amd/host/blob_layout.h), without a device: the whole array as the upload lays
// it out, and the step yh_update_shape makes for one shape. The properties are checked from the rule as include/yhair.h and DESIGN.md state
// it; the numbers are checked against tests/golden/blob_layout.txt (argv[1]), which the code that blob_layout.h replaced wrote.
#include <algorithm>
#include <fstream>
#include <string>

#include "blob_layout.h"
#include "blob_layout_cases.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) printf("FAILED line %d (%s): %s\n", __LINE__, what, #cond), failures++; \
  } while (0)

namespace {
struct Region {
  long long begin, end;  // [begin, end) in units
};
}  // namespace

static void check_layout(const LayoutCase& c, std::vector<std::string>& lines) {
  const char*            what = c.name;
  std::vector<BlobShape> in;
  for (const CaseShape& s : c.shapes) in.push_back({s.lines, s.num_prims, {s.count[0], s.count[1], s.count[2]}});
  BlobLayout B;
  long long  at = -1;
  const int  rc = blob_layout(c.scene_wide, c.num_objects, in.data(), (int)in.size(), B, &at);
  std::vector<RegionLine> regions;
  for (const BlobRegions& r : B.shapes) regions.push_back({r.test_off, {r.node_off[0], r.node_off[1], r.node_off[2]}});
  lines.push_back(layout_line(c.name, rc, at, B.lane_units, B.units, regions));
  CHECK(rc == c.expect);
  CHECK((rc == YH_BLOB_LEAF_OFFSETS) == (c.expect == 1) && (rc == YH_BLOB_NODE_OFFSETS) == (c.expect == 2));
  if (rc == YH_BLOB_LEAF_OFFSETS) CHECK(at >= (1ll << 27));
  if (rc == YH_BLOB_NODE_OFFSETS) CHECK(at >= (1ll << 30));
  if (rc) return;
  CHECK(B.units < (1ll << 30));
  const size_t n = in.size();
  // every region in the order the array has them: scene nodes, test records, then the nodes width by width
  std::vector<Region> all;
  if (c.scene_wide) all.push_back({0, 4ll * c.num_objects});  // room for as many 4-wide scene nodes as there are objects
  long long tests_end = 0, width_end[3] = {0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const long long len = (long long)in[i].num_prims * (in[i].lines ? 1 : 2);
    all.push_back({B.shapes[i].test_off, B.shapes[i].test_off + len});
    tests_end = B.shapes[i].test_off + len;
  }
  CHECK(tests_end + 4 <= (1ll << 27));
  for (int w = 0; w < 3; w++)
    for (size_t i = 0; i < n; i++) {
      const long long off = B.shapes[i].node_off[w], len = (long long)(4 << w) * in[i].count[w];
      CHECK(off % 4 == 0);  // on a 128-byte line
      all.push_back({off, off + len});
      width_end[w] = off + len;
    }
  for (size_t k = 1; k < all.size(); k++) CHECK(all[k].begin >= all[k - 1].end);  // no overlap, in this order
  CHECK(all[0].begin == 0);
  // four units of slack behind the last test record, behind the last 4-wide node (where the one-lane kernels' range ends) and behind
  // the array's last node; the 8-wide nodes are followed by the 16-wide ones directly (both on 128-byte lines), or by that last slack
  CHECK(B.shapes[0].node_off[0] >= tests_end + 4 && B.shapes[0].node_off[0] < tests_end + 8);
  CHECK(B.lane_units == width_end[0] + 4);
  CHECK(B.shapes[0].node_off[1] >= B.lane_units && B.shapes[0].node_off[1] < B.lane_units + 4);
  CHECK(B.shapes[0].node_off[2] == width_end[1]);
  CHECK(B.units == width_end[2] + 4);
  CHECK(B.units >= all.back().end + 4);
  long long furthest = 0;
  for (size_t i = 0; i < n; i++) furthest = std::max(furthest, blob_lane_end(B.shapes[i].node_off[0], in[i].count[0]));
  CHECK(furthest == B.lane_units);  // (the edits' way of stating it agrees with the upload's)
}

static void check_growth(const GrowthCase& c, std::vector<std::string>& lines) {
  const char* what = c.name;
  BlobGrowth  G;
  const int   rc = blob_growth(c.old_units, c.old_off, c.old_room, c.count, G);
  lines.push_back(growth_line(c.name, rc, G.units, G.off, G.room));
  CHECK(rc == c.expect);
  CHECK((rc != YH_BLOB_OK) == (G.units >= (1ll << 30)));
  long long end = c.old_units;
  for (int w = 0; w < 3; w++) {
    if (c.count[w] <= c.old_room[w]) {  // it still fits: where it was, with the room it had
      CHECK(G.off[w] == c.old_off[w] && G.room[w] == c.old_room[w]);
      continue;
    }
    CHECK(G.off[w] % 4 == 0 && G.off[w] >= end && G.off[w] < end + 4);  // the aligned end
    CHECK(G.room[w] == c.count[w] + c.count[w] / 8);
    end = G.off[w] + (long long)(4 << w) * G.room[w] + 4;  // (slack behind it, as the upload leaves)
  }
  CHECK(G.units == end);
}

int main(int argc, char** argv) {
  std::vector<std::string> lines;
  for (const LayoutCase& c : layout_cases) check_layout(c, lines);
  for (const GrowthCase& c : growth_cases) check_growth(c, lines);
  const char* what = "lane_units";
  {  // lane_units follows the furthest 4-wide region: shape 1's moves behind the old end
    const long long off_a = 1004, off_b = 2340;
    const int       room_a = 333, room_b = 12;
    CHECK(std::max(blob_lane_end(off_a, room_a), blob_lane_end(off_b, room_b)) == 2340 + 48 + 4);
    CHECK(std::max(blob_lane_end(off_a, room_a), blob_lane_end(900, room_b)) == 1004 + 4 * 333 + 4);
  }
  what = "golden";
  if (argc > 1) {
    std::ifstream            in(argv[1]);
    std::vector<std::string> want;
    for (std::string line; std::getline(in, line);)
      if (!line.empty() && line[0] != '#') want.push_back(line);
    CHECK(want.size() == lines.size());
    for (size_t k = 0; k < std::min(want.size(), lines.size()); k++)
      if (want[k] != lines[k]) printf("FAILED: golden line %zu\n  want %s\n  have %s\n", k, want[k].c_str(), lines[k].c_str()), failures++;
  } else {
    for (const std::string& l : lines) puts(l.c_str());
    printf("FAILED: no golden file given\n"), failures++;
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("all checks passed\n");
  return 0;
}
