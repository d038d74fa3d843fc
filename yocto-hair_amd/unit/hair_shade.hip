// hair_shade.hip — the hair path of a shaded hit at unit level (gfx950), in the arithmetic every sample-loop kernel but csrc/exact.hip
// runs (YH_HAIR_FAST = 1): yh_hair_shade_batch with exact = 0, form 0 (a quad per row, as k_trace) and form 1 (a lane per row, as
// k_stream). A translation unit of its own, outside csrc/: the sample-loop kernels compile to exactly the code they compiled to without it.
#define YH_HAIR_SHADE_KERNEL k_hair_shade
#define YH_HAIR_SHADE_LAUNCH yhk_hair_shade
#include "launchers.h"
#include "hair_shade.h"
