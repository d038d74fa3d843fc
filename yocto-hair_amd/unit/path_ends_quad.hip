// path_ends_quad.hip — the start and the end of a path with a quad per row (gfx950): form 0 of yh_path_ends_batch, what the quad sample
// loops run (path_begin with the quad form of sample_camera, path_continue, path_end). A translation unit of its own, outside csrc/, as
// unit/volume_quad.hip.
#define YH_PATH_ENDS_KERNEL k_path_ends_quads
#define YH_PATH_ENDS_LAUNCH yhk_path_ends_quads
#include "launchers.h"
#include "path_ends.h"
