// ttcr_amd/csrc/fsm_fast.hip -- translation unit of the sweep kernels with tolerance-grade arithmetic; see fsm_fast_api.h.
#include "fsm_fast_api.h"

namespace ttcr_amd {

// Every tolerance-grade kernel there is: whole-iteration launches of fp32 grids (T, DIM, H, NS, chunk[, PRE], AR = 1)
using FastSweepKernels = SweepKernels<
#ifndef FSM_FAST_MIN   // (tuning builds: the lone-source kernels only)
    // WENO stage, one field per workgroup: 3-D on chunks of 16 and of 8, 2-D (PRE always)
    WholeIteration<float, 3, 2, 1, 16, 1>, WholeIteration<float, 3, 2, 1, 8, 1>, WholeIterationPre<float, 2, 2, 1, 16, true, 1>,
#endif
    // first order, 3-D, one field per workgroup (no PRE on chunks of 16)
    WholeIterationPre<float, 3, 1, 1, 16, false, 1>
#ifndef FSM_FAST_MIN
    // ... source pairs; first order, 2-D
    , WholeIteration<float, 3, 1, 2, 8, 1>, WholeIterationPre<float, 2, 1, 1, 16, true, 1>
#endif
    >;

bool fsm_fast_sweep_exists(const SweepPlan& p) { return FastSweepKernels::has(p); }
bool fsm_fast_sweep(const SweepPlan& p, const PersistArgs<float>& pa, hipStream_t stream) { return FastSweepKernels::run(p, pa, stream); }

}  // namespace ttcr_amd
