// hair_shade_exact.hip — the same rows in the hair BSDF's EXACT arithmetic (yh_trace_params::hair_exact, csrc/exact.hip): the body of
// hair_shade.h compiled with YH_HAIR_FAST = 0 under a kernel name of its own. The quad form only (yh_hair_shade_batch with exact = 1,
// form 0): a launch with hair_exact runs the quad kernel and no other.
#define YH_HAIR_FAST 0
#define YH_HAIR_SHADE_KERNEL k_hair_shade_exact
#define YH_HAIR_SHADE_LAUNCH yhk_hair_shade_exact
#include "launchers.h"
#include "hair_shade.h"
