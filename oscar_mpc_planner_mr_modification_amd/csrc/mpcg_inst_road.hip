// Built-in instances: T-MPC++ unicycle with the two road-boundary halfspaces
// (add_halfspaces 2: n_lin = max_obstacles + 2).
#include "mpcg_instance.h"

MPCG_DEFINE_INSTANCE(20, 10, 8, 0, 5, 0)   // C2R: C2 plus the road rows
MPCG_DEFINE_INSTANCE(30, 6, 4, 0, 5, 0)    // JSR: the jackalsimulator solver plus the road rows
