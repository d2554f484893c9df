// From a SweepPlan (fsm_sweep_plan.h) to the instantiation of fsm_sweep_persistent it names.  A translation unit lists the kernels it
// holds as one SweepKernels<...> type (fsm_capi.hip: the exact ones, fsm_fast.hip: the tolerance-grade ones); has() on that list says
// whether the plan names one of them, run() launches it.
#pragma once
#include "fsm_kernels.h"
#include "fsm_sweep_plan.h"

namespace ttcr_amd {

template <typename T, int DIM, int H, int NS, int CH, bool SKIP, bool XS, bool PRE, int AR>
struct SweepKernel {
    using C = TileCfg<T, DIM>;
    static bool has(const SweepPlan& p) {
        return p.persistent && p.f32 == (sizeof(T) == 4) && p.dim == DIM && p.PJ == C::PJ && p.PK == C::PK && p.H == H && p.NS == NS &&
               p.chunk == CH && (p.skip != 0) == SKIP && p.XS == XS && p.PRE == PRE && p.AR == (AR != 0);
    }
    static bool run(const SweepPlan& p, const PersistArgs<T>& pa, hipStream_t stream) {
        if (!has(p)) return false;
        fsm_sweep_persistent<T, C::PJ, C::PK, CH, DIM == 3, SKIP, H, NS, XS, PRE, AR><<<dim3(p.wgs), dim3(p.block), p.dyn_lds, stream>>>(pa);
        return true;
    }
};

template <typename... K>
struct SweepKernels {
    static bool has(const SweepPlan& p) { return (... || K::has(p)); }
    template <typename T>
    static bool run(const SweepPlan& p, const PersistArgs<T>& pa, hipStream_t stream) { return (... || K::run(p, pa, stream)); }
};

// The families a list is written in.  Whole-iteration launch: with and without exact skipping ...
template <typename T, int DIM, int H, int NS, int CH, bool PRE, int AR = 0>
using WholeIterationPre = SweepKernels<SweepKernel<T, DIM, H, NS, CH, true, true, PRE, AR>, SweepKernel<T, DIM, H, NS, CH, false, true, PRE, AR>>;
// ... each with and without the upwind counters sampled one chunk ahead
template <typename T, int DIM, int H, int NS, int CH, int AR = 0>
using WholeIteration = SweepKernels<SweepKernel<T, DIM, H, NS, CH, true, true, true, AR>, SweepKernel<T, DIM, H, NS, CH, true, true, false, AR>,
                                    SweepKernel<T, DIM, H, NS, CH, false, true, true, AR>, SweepKernel<T, DIM, H, NS, CH, false, true, false, AR>>;
// ... and the launch per sweep as well
template <typename T, int DIM, int H, int NS, int CH>
using EveryLaunch = SweepKernels<WholeIteration<T, DIM, H, NS, CH>, SweepKernel<T, DIM, H, NS, CH, true, false, false, 0>,
                                 SweepKernel<T, DIM, H, NS, CH, false, false, false, 0>>;

}  // namespace ttcr_amd
