// point_lane.hip — the shading point with one lane per row (gfx950): form 1 of yh_point_batch, what k_stream's shading stage runs
// (YH_LANE forms). A translation unit of its own, outside csrc/, as unit/volume_lane.hip.
#define YH_LANE 1
#define YH_POINT_KERNEL k_point_lanes
#define YH_POINT_LAUNCH yhk_point_lanes
#include "launchers.h"
#include "point_shade.h"
