// group emission (policy.hpp EmitPT<true>): the light units for every selected witness of a group at once
#include "g_units.hpp"
POB_DEFINE_G_LAUNCH(launch_g_emit_group_light, EmitGroupP, FAM_LIGHT, 4)
