// point_quad.hip — the shading point with a quad per row (gfx950): forms 0 and 2 of yh_point_batch, what the quad kernels' path_step /
// shade_step run between the closest hit and the lobes, and the small kernel that inverts a shape's leaf order for the batch. A
// translation unit of its own, outside csrc/, as unit/volume_quad.hip.
#define YH_POINT_KERNEL k_point_quads
#define YH_POINT_LAUNCH yhk_point_quads
#include "launchers.h"
#include "point_shade.h"
