// volume_lane.hip — the homogeneous-medium code with one lane per row (gfx950): form 1 of yh_volume_batch, what k_stream's shading stage
// runs (YH_LANE forms: the medium travels through the path's slot). A translation unit of its own, outside csrc/, as unit/lights_lane.hip.
#define YH_LANE 1
#define YH_VOLUME_KERNEL k_volume_lanes
#define YH_VOLUME_LAUNCH yhk_volume_lanes
#include "launchers.h"
#include "volume_shade.h"
