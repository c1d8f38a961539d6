// group emission (policy.hpp EmitPT<true>): the BN254 units -- the longest compile of the build, alone in its translation unit
#include "g_units.hpp"
POB_DEFINE_G_LAUNCH(launch_g_emit_group_heavy, EmitGroupP, FAM_HEAVY, 2)
