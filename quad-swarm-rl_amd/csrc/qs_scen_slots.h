// qs_scen_slots.h - the slots of the per-environment scenario state (scen_int / scen_real; qs_scenarios.h works on them).  Plain C++:
// qs_lds_layout.h sizes the LDS copy of that state by the two counts, on the host and without a HIP header.
#pragma once
namespace qs {
// scen_int slots
enum { SI_PERIOD = 0, SI_SCEN, SI_FORM, SI_PER_LAYER, SI_INCREASE, SI_BEZ_VALID, SI_CONSTRUCTED, SI_HAVE_SPAWN, SI_COUNT = 8 };
// scen_real slots
enum { SR_C1 = 0, SR_C2 = 3, SR_LO = 6, SR_HI, SR_SIZE, SR_LAYER, SR_SPEED, SR_BEZ = 11, SR_END = 20, SR_METRIC = 23, SR_COUNT = 24 };
}  // namespace qs
