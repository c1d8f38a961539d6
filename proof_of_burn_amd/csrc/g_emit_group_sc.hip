// group emission (policy.hpp EmitPT<true>): the SubstringCheck units; U_SC_RANGE's inverses are every witness' own here (circuits.hpp)
#include "g_units.hpp"
POB_DEFINE_G_LAUNCH(launch_g_emit_group_sc, EmitGroupP, FAM_BIT(F_SC), 4)
