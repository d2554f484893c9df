// ttcr_amd/csrc/fsm_fast_api.h -- what the host side (fsm_capi.hip) sees of the sweep kernels with tolerance-grade arithmetic
// (option "arith" = 1: update3_fast / update2_fast / weno_axis_fast of fsm_kernels.h instead of the reference's fp64 arithmetic).  They are the
// AR = 1 instantiations of fsm_sweep_persistent -- same arguments, synchronisation words, ticket lists and launch geometry as the
// exact kernels the host would launch otherwise -- compiled in a translation unit of their own (fsm_fast.hip).
#pragma once
#include "fsm_sweep_dispatch.h"

namespace ttcr_amd {

// the AR = 1 instantiation the plan names: whether there is one, and its launch (false: there is none)
bool fsm_fast_sweep_exists(const SweepPlan& p);
bool fsm_fast_sweep(const SweepPlan& p, const PersistArgs<float>& pa, hipStream_t stream);

}  // namespace ttcr_amd
