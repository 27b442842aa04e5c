// Missing-observation build of bsim_wobs.hip: a NaN in obs is an observation that was not made and its term is left out of
// log g (include/psvo_hip.h: psvo_bsim_forward_wobs_missing, psvo_bsim_backward_wobs_missing; 1 <= Dy <= 32).  See PSVO_MS in
// bsim_wobs.hip.
#define PSVO_MS 1
#include "bsim_wobs.hip"
