// path_ends_lane.hip — the start and the end of a path with one lane per row (gfx950): form 1 of yh_path_ends_batch, what k_stream's finish
// stage runs (the four draws and sample_camera_lane, path_continue, path_end). A translation unit of its own, outside csrc/, as
// unit/volume_lane.hip.
#define YH_LANE 1
#define YH_PATH_ENDS_KERNEL k_path_ends_lanes
#define YH_PATH_ENDS_LAUNCH yhk_path_ends_lanes
#include "launchers.h"
#include "path_ends.h"
