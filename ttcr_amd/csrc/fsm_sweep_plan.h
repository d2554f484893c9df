// Which sweep kernel a launch runs, with what geometry, and what it is called: plain host arithmetic, no HIP and no grid object
// (GridT::sweep_plan and the device-free C entry ttcr_fsm_sweep_plan both call it; tests/test_sweep_plan.py checks what it promises).
// Every rule that picks a template argument of fsm_sweep_persistent / fsm_sweep_tile stands here once; fsm_sweep_dispatch.h maps the
// SweepPlan to the instantiation, fsm_sweep_name prints the name ttcr_fsm_last_kernel reports, and SweepPlan::operator== keys the
// captured launch of GridT::run_iteration.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <type_traits>

// tile shapes (threads = PJ*PK); see DESIGN.md section 4 for the LDS budget
template <typename T, int DIM> struct TileCfg;
#ifndef FSM_PJ3
#define FSM_PJ3 16
#endif
#ifndef FSM_PK3
#define FSM_PK3 16
#endif
template <> struct TileCfg<float, 3> { static constexpr int PJ = FSM_PJ3, PK = FSM_PK3, BL = 16; };
template <> struct TileCfg<double, 3> { static constexpr int PJ = 16, PK = 8, BL = 16; };
#ifndef FSM_PJ2
#define FSM_PJ2 64
#endif
#ifndef FSM_CHUNK2
#define FSM_CHUNK2 16
#endif
#ifndef FSM_CHUNK3
#define FSM_CHUNK3 8
#endif
template <> struct TileCfg<float, 2> { static constexpr int PJ = FSM_PJ2, PK = 1, BL = 32; };
template <> struct TileCfg<double, 2> { static constexpr int PJ = FSM_PJ2, PK = 1, BL = 32; };
// chunk length of the persistent kernel
template <typename T, int DIM> struct ChunkCfg { static constexpr int C = DIM == 3 ? FSM_CHUNK3 : FSM_CHUNK2; };

// ---- tuning values -------------------------------------------------------------------------------------------------------------
// Read from the environment once, when a grid is created (fsm_sweep_tuning); every default stands beside the measurements behind it.
struct SweepTuning {
    // source pairs (fields interleaved, marched together) for the first-order 3-D solver only.  The one-wave 2-D
    // patches issue in order, a second source doubles the instructions of a level and buys nothing (4096^2:
    // 16 sources 28.0 -> 20.8 ms, 64 sources 35.8 -> 28.9 ms, 256 sources 112 -> 87 ms unpaired); the WENO stage
    // is bound by its arithmetic, and pairs cost it a resident wave (256^3: 2 sources 761 -> 483 ms, 8 sources
    // 1208 -> 973 ms, 16 sources 1740 -> 1672 ms, 64 sources 5986 -> 6221 ms).  profiles/r02/pairing.txt
    // Round 4, with exact skipping on by default for batches: on a model where most chunks are skipped, pairs only pay once the
    // chip has more work units than it can keep in flight -- a chunk of a pair is evaluated when EITHER source needs it and a
    // pair's level is the longer chain; on a model where most chunks are evaluated they pay from 4 sources on.
    // 512^3 (1 024 patches), ms per sweep-iteration paired / unpaired, gradient model (66 % of the updates skipped):
    //   2 sources 10.1 / 8.1, 4: 12.0 / 10.6, 8: 17.3 / 16.2, 16: 27.2 / 30.2, 32: 45.9 / 58.4; 256^3: 8 sources 5.7 / 4.5, 16: 6.5 / 6.1
    // ms per solve, random 16^3-block model (8-11 iterations, 75-83 % evaluated):
    //   2 sources 109.9 / 110.5, 4: 191 / 203, 8: 314 / 372, 16: 556 / 710      (profiles/r04/README.md)
    // So: pairs when slots x patches of a sweep exceed pair_units_min = 6 144 (512^3: from 8 sources on, where the smooth model
    // loses 7 % and the rough one gains 18 %; below, the smooth model gains 13-25 % and the rough one loses 0-6 %).
    long long pair_units_min = 6144;   // TTCR_FSM_PAIR_UNITS (tuning only)
    int pair = -1;                     // TTCR_FSM_PAIR: 0 / 1 pins the layout of every grid with two slots or more (-1: unset)
    // (with chunk-shaped dirty bits the 8-source legs of the bench evaluate 0.25 on the gradient model and 0.67 on the rough one, one field per
    // workgroup; with the slab mask it was 0.28 and 0.83 in pairs, and the thresholds 0.55 / 0.70 -- which left the rough model on the slower layout)
    double layout_lo = 0.45, layout_hi = 0.55;   // pairs -> one field per workgroup below lo, back above hi (TTCR_FSM_LAYOUT_LO / _HI: tests, tuning)
    int weno_ch4_min = 8;    // pair layout: slot groups from which the 3-D WENO stage uses chunks of 4 levels
    int weno_c16_below = 3;  // one field per workgroup: batch entries below which the 3-D WENO stage uses chunks of 16 levels (option lone_chunk = 16)
    int f64_c16_below = 5;   // ... below which the fp64 first-order 3-D sweeps do
    int pre_min = 2;         // 3-D: slot groups in a batch from which the upwind counters are sampled one chunk ahead (PRE)
    // extra (unused) dynamic LDS per workgroup of the whole-iteration launch: caps the resident workgroups per CU.  A lone
    // source is bound by the dependent chain of a marching unit, and a unit that shares its CU's SIMDs with another
    // marching unit runs that chain slower (TTCR_FSM_XS_LDS=bytes, TTCR_FSM_XS_LDS_BELOW=groups; 0: off)
    // Measured, 512^3: one source 8.49 -> 7.37 ms per sweep-iteration with two workgroups per CU instead of four (7.14 with
    // the counters sampled ahead as well), one source pair 10.5 -> 9.96; one per CU 9.95 (too few units in flight);
    // from two slot groups on, and for the 2-D and WENO kernels, the cap does not pay (profiles/r02/occupancy_cap.txt).
    size_t xs_lds_bytes = 40000;
    int xs_lds_below = 2;
    int time_order_below = 1 << 30; // fewer batch entries (slot groups / slots) than this in a batch: the whole-iteration launch hands its units out in the
                               // order of their expected start times instead of sweep by sweep (build_persistent_lists).  Until round 5: 17 -- with
                               // the kernels of round 5 the start-time order wins at every size measured (512^3, two sweep-iterations: 64 sources
                               // 169.8 -> 166.8 ms, 34 sources 99.6 -> 96.0, 48: 134.4 -> 133.8; rough model, 64 sources to convergence 2 004 ->
                               // 1 917 ms; 256^3 x 24 sources 8.17 -> 7.67 ms per sweep-iteration; 2-D 4096^2 x 64 18.5 -> 18.4;
                               // profiles/r05/experiment_ticket_order.txt)
    // Exact skipping of chunks / units / sweeps that cannot change a node: on wherever it was measured to pay
    // (profiles/r03/skip_sweep.txt).  What it saves is work, what it costs is a little of every chunk's time: a win once
    // the chip is busy (512^3: from two slot groups on, 1.13x ... 1.7x at 32 groups), a loss of 1-15 % where a 3-D solve is
    // bound by the dependent chain of its units anyway (a lone source or pair; 256^3 and smaller up to 8 sources).  The
    // WENO stage gains at every batch size (its chunks are expensive), and so do the one-wave patches of the 2-D solver
    // (1.03x ... 1.19x from 1 to 64 sources on 1024^2 ... 8192^2 nodes, although the SKIP kernels do not follow the
    // previous sweep up the columns).  TTCR_FSM_SKIP_UNITS: work units per sweep from which the first-order 3-D sweeps skip.
    int skip_units_min = 2048;
    // Round 6: between 1 024 and 2 048 units (a lone 512^3 source, 2 - 4 sources at 384^3 ...) whether skipping pays depends on the MODEL -- 512^3,
    // one source, ms per solve without / with: gradient model 13.3 / 12.8 (arith = 1: 10.9 / 9.6), rough 16^3-block model 65.5 / 68.2 (52.2 / 54.9);
    // 384^3: 9.4 / 9.2 and 32.5 / 35.1 (profiles/r06/lone_skip_models.txt).  Such fp32 launches follow the evaluated fraction of the grid's last
    // skipping solve: on while it stayed below 0.6, off above, and tried again after eight solves without.
    int skip_probe_min = 1024;
    int persist_wgs = 2048;   // workgroups of a sweep launch (each takes units until none is left): 8 per CU; 0: one per unit (TTCR_FSM_WGS)
    bool skip_all_dirty = false;   // TTCR_FSM_SKIP_ALL_DIRTY (tuning / bisecting): the SKIP kernels take every chunk for dirty
    bool no_sw = false;            // TTCR_FSM_NO_SW (tuning / bisecting): no whole-sweep shortcut
};

// The tuning values of a grid whose device keeps `wg_cap` workgroups of a sweep launch busy (8 per CU), as the environment sets them.
inline SweepTuning fsm_sweep_tuning(int wg_cap) {
    SweepTuning t;
    t.persist_wgs = wg_cap;
    const auto num = [](const char* name, auto& v) {
        if (const char* e = std::getenv(name)) v = static_cast<std::decay_t<decltype(v)>>(std::atoll(e));
    };
    num("TTCR_FSM_PAIR_UNITS", t.pair_units_min);   // tuning only, like every variable below but TTCR_FSM_PAIR and TTCR_FSM_XS_LDS*
    if (const char* e = std::getenv("TTCR_FSM_PAIR")) t.pair = std::atoi(e) != 0;
    if (const char* e = std::getenv("TTCR_FSM_LAYOUT_LO")) t.layout_lo = std::atof(e);
    if (const char* e = std::getenv("TTCR_FSM_LAYOUT_HI")) t.layout_hi = std::atof(e);
    num("TTCR_FSM_WENO_CH4_MIN", t.weno_ch4_min);
    num("TTCR_FSM_WENO_C16_BELOW", t.weno_c16_below);
    num("TTCR_FSM_F64_C16_BELOW", t.f64_c16_below);
    num("TTCR_FSM_TIME_ORDER_BELOW", t.time_order_below);
    num("TTCR_FSM_PRE_MIN", t.pre_min);
    num("TTCR_FSM_SKIP_UNITS", t.skip_units_min);
    num("TTCR_FSM_SKIP_PROBE_UNITS", t.skip_probe_min);
    num("TTCR_FSM_WGS", t.persist_wgs);
    num("TTCR_FSM_XS_LDS", t.xs_lds_bytes);
    num("TTCR_FSM_XS_LDS_BELOW", t.xs_lds_below);
    t.skip_all_dirty = std::getenv("TTCR_FSM_SKIP_ALL_DIRTY") != nullptr;
    t.no_sw = std::getenv("TTCR_FSM_NO_SW") != nullptr;
    return t;
}

// The options of a grid that choose among the sweep kernels (ttcr_fsm_set_option), with the defaults the environment gives them.
struct SweepOptions {
    int mode = 2;         // 2: whole iteration in one launch, 1: one launch per sweep, 0: one launch per tile wavefront
    int skip = -1;        // exact skipping: 1 on, 0 off, -1 where it was measured to pay (fsm_skip_default)
    int lone_chunk = 16;  // levels per chunk of the 3-D kernels with one field per workgroup (8 or 16)
    int arith = 0;        // 0 the reference's arithmetic, 1 tolerance-grade fp32 without the WENO stage, 2 the WENO stage too
};
inline SweepOptions fsm_sweep_options() {
    SweepOptions o;
    if (const char* e = std::getenv("TTCR_FSM_SKIP")) o.skip = std::atoi(e);
    if (const char* e = std::getenv("TTCR_FSM_MODE")) o.mode = std::atoi(e);
    if (const char* e = std::getenv("TTCR_FSM_LONE_CHUNK")) o.lone_chunk = std::atoi(e) == 8 ? 8 : 16;   // tuning only
    if (const char* e = std::getenv("TTCR_FSM_ARITH")) o.arith = std::max(0, std::min(2, std::atoi(e)));
    return o;
}

// Pairs (NS = 2) or one field per workgroup (NS = 1) for a grid of n_slots slots and `patches` patches per sweep, and whether the grid
// is in the window where its layout follows the model (see pair_units_min).
// Round 6: between the threshold and 2.5 x the threshold (512^3: 8 ... 15 slots) which layout is faster depends on the MODEL --
// smooth (most chunks skipped): one field per workgroup on 16-level chunks, 15.2 against 17.2 ms per sweep-iteration for 8 sources;
// rough (most chunks evaluated): pairs, 311 against 360 ms per solve.  Both layouts take the same memory, so such a grid follows
// the evaluated fraction of its last call that restarted every slot (choose_layout); option "pair_layout" pins it.
inline int fsm_pair_layout(const SweepTuning& t, int dim, bool weno, int n_slots, long long patches, bool* window) {
    if (t.pair >= 0) { *window = false; return (t.pair && n_slots >= 2) ? 2 : 1; }
    const int ns = (n_slots >= 2 && dim == 3 && !weno && (long long)n_slots * patches > t.pair_units_min) ? 2 : 1;
    *window = ns == 2 && (long long)n_slots * patches <= (5 * t.pair_units_min) / 2;
    return ns;
}

// words of chunk-shaped dirty bits per unit (chunks of 8 levels or more; fsm_chunk_dirty.h)
inline int fsm_cdirty_wpu(int NF, int PJ, int PK) { return ((NF + 2 * (PJ + PK)) / 8 + 4) / 32 + 1; }
// launches per sweep direction of the tile-wavefront kernel (levels of BL nodes over every patch's window)
inline int fsm_tile_launches(int NF, int NJ, int NK, int npj, int npk, int BL) {
    return ((NJ - 1) + (NK - 1) + NF - 1 + (npj + npk - 2) * (BL - 1)) / BL + 1;
}

// ---- what the plan depends on ---------------------------------------------------------------------------------------------------
struct SweepFacts {
    // the grid
    int dim = 3;
    bool f32 = true, weno = false;
    bool rot45 = false;       // 2-D rotated template with dx == dz: sweep45 follows every first-order sweep
    int PJ = 16, PK = 16, BL = 16, C0 = 8;   // TileCfg, ChunkCfg
    int n_patches = 0, NF = 0, NJ = 0, NK = 0, nbf = 0, cdirty_wpu = 1, n_launch = 0;
    int slab_bits = 0, cd_words = 0;   // F bricks a SKIP kernel's mask holds, words of dirty bits per unit it holds (fsm_kernels.h)
    int NS = 1;               // fields per workgroup now (fsm_pair_layout, choose_layout)
    SweepOptions opt;
    // the state
    int stage = 0;            // 0: first-order sweeps, 1: WENO3 sweeps (persistent kernel only)
    bool probe_skip = true;   // what a launch in the probe window does now (see skip_probe_min)
    int batch = 1;            // batch entries (slot groups / slots) swept together
};
// the tile and chunk sizes of a grid of T in `dim` dimensions
template <typename T>
inline void fsm_sweep_tiles(SweepFacts& f, int dim) {
    using C3 = TileCfg<T, 3>;
    using C2 = TileCfg<T, 2>;
    f.dim = dim;
    f.f32 = sizeof(T) == 4;
    f.PJ = dim == 3 ? C3::PJ : C2::PJ; f.PK = dim == 3 ? C3::PK : C2::PK; f.BL = dim == 3 ? C3::BL : C2::BL;
    f.C0 = dim == 3 ? ChunkCfg<T, 3>::C : ChunkCfg<T, 2>::C;
}

// Tolerance-grade arithmetic (fp32 grids).  arith = 1: the first-order sweeps of grids WITHOUT the WENO stage -- within north_star's
// 1e-5 s RMS of the reference.  A grid with the WENO stage keeps the reference's arithmetic in BOTH stages under arith = 1: the WENO
// iteration amplifies differences of an ulp in its input field to 1e-3 s (measured, profiles/r06/weno_sensitivity.txt: the exact WENO
// stage behind a tolerance-grade first-order stage ends 4e-5 s RMS / 4e-3 s max away from the reference) -- only the bit-identical
// first-order field reproduces the reference there.  arith = 2: both stages of such grids as well, outside that bound, for callers
// who take the WENO stage's own sensitivity as their tolerance.
inline bool fsm_fast_arith(const SweepFacts& f) { return f.f32 && (f.opt.arith == 2 || (f.opt.arith == 1 && !f.weno)); }
inline bool fsm_persistent(const SweepFacts& f) { return f.opt.mode >= 1 || f.stage == 1; }
inline long long fsm_units_per_sweep(const SweepFacts& f) { return (long long)f.n_patches * f.batch; }
inline bool fsm_in_probe_window(const SweepFacts& f, const SweepTuning& t) {
    const long long u = fsm_units_per_sweep(f);
    return f.dim == 3 && f.f32 && u >= t.skip_probe_min && u < t.skip_units_min;
}
inline int fsm_skip_default(const SweepFacts& f, const SweepTuning& t) {
    if (f.dim != 3) return 1;
    if (f.stage == 1) return 1;
    if (fsm_in_probe_window(f, t)) return f.probe_skip ? 1 : 0;
    return fsm_units_per_sweep(f) >= t.skip_units_min ? 1 : 0;
}
// the rotated-template sweeps change nodes without stamping their bricks: no skipping next to them
inline bool fsm_skip(const SweepFacts& f, const SweepTuning& t) {
    const int on = f.opt.skip < 0 ? fsm_skip_default(f, t) : f.opt.skip;
    // (the SKIP kernels pack a level count and 8 flag bits into one progress word, and keep one mask bit per F brick)
    // (... and, first-order 3-D sweeps, one dirty bit per chunk of a unit in cd_words words: true of every grid with that many F bricks)
    const bool fits = (long long)f.NF + f.NJ + f.NK < (1ll << 22) && f.nbf <= f.slab_bits && (f.dim != 3 || f.cdirty_wpu <= f.cd_words);
    return on != 0 && fits && !(f.dim == 2 && f.rot45 && !f.weno);
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
struct SweepPlan {
    enum Tickets { PER_SWEEP = 0, XS_BY_SWEEP = 1, XS_BY_TIME = 2 };   // d_order / d_order_xs[stage][0] / d_order_xs[stage][1]
    bool persistent = true;   // fsm_sweep_persistent, else fsm_sweep_tile (one launch per tile wavefront)
    bool arith_needs_xs = false;   // no plan: tolerance-grade arithmetic asked for without whole-iteration launches (a ValueError)
    bool f32 = true;
    int dim = 3, PJ = 16, PK = 16, BL = 16;
    int H = 1, chunk = 8, NS = 1;   // halo width (stage + 1), levels per chunk, fields per workgroup
    int skip = 0;                   // template SKIP; 2: on, every chunk taken for dirty (PersistArgs::skip)
    bool XS = true, PRE = false, AR = false;
    bool sw = true;                 // the whole-sweep tallies are handed to the kernel
    size_t dyn_lds = 0;
    unsigned wgs = 0, block = 0;    // workgroups (persistent kernels) and threads of a launch
    int tickets = XS_BY_TIME;
    int batch = 0;
    long long launches = 0;         // per sweep-iteration
    bool operator==(const SweepPlan& o) const {
        return persistent == o.persistent && arith_needs_xs == o.arith_needs_xs && f32 == o.f32 && dim == o.dim && PJ == o.PJ && PK == o.PK &&
               BL == o.BL && H == o.H && chunk == o.chunk && NS == o.NS && skip == o.skip && XS == o.XS && PRE == o.PRE && AR == o.AR &&
               sw == o.sw && dyn_lds == o.dyn_lds && wgs == o.wgs && block == o.block && tickets == o.tickets && batch == o.batch &&
               launches == o.launches;
    }
    bool operator!=(const SweepPlan& o) const { return !(*this == o); }
};

inline SweepPlan fsm_sweep_plan(const SweepFacts& f, const SweepTuning& t) {
    SweepPlan p;
    const int ndir = f.dim == 3 ? 8 : 4;
    const bool fast = fsm_fast_arith(f);
    p.f32 = f.f32; p.dim = f.dim; p.PJ = f.PJ; p.PK = f.PK; p.BL = f.BL;
    p.NS = f.NS; p.batch = f.batch; p.block = (unsigned)(f.PJ * f.PK);
    p.persistent = fsm_persistent(f);
    p.XS = p.persistent && f.opt.mode == 2;
    p.arith_needs_xs = fast && !p.XS;
    if (!p.persistent) {   // (the tile kernel has one instantiation per precision and dimension, and no workgroup count of its own)
        p.H = 1; p.chunk = f.BL; p.XS = false; p.tickets = SweepPlan::PER_SWEEP; p.sw = false;
        p.launches = (long long)ndir * f.n_launch;
        return p;
    }
    p.H = f.stage + 1;
    p.skip = fsm_skip(f, t) ? (t.skip_all_dirty ? 2 : 1) : 0;
    p.sw = !t.no_sw;
    // The 3-D WENO stage exists with two chunk lengths: 8 levels (the kernel is latency bound with few
    // sources: fewer chunk boundaries) and 4 levels (157 instead of 208 VGPRs in pair mode, no spills, three
    // waves per SIMD: +14 % throughput once >= 8 slot groups are swept together).  Same results either way.
    // (pair layout only: with one field per slot -- the default of weno grids since round 2 -- the 8-level chunks are
    // 2-4 % faster at every batch size, profiles/r02/weno_chunk.txt)
    p.chunk = (p.H == 2 && f.dim == 3 && f.NS == 2 && f.batch >= t.weno_ch4_min && f.C0 == 8) ? 4 : f.C0;
    // One field per workgroup (lone sources, batches below the pairing threshold): such launches are bound by the chains of their
    // chunks rather than by registers, and chunks of 16 levels halve the staging, the write-back and the hand-offs per level --
    // ms per sweep-iteration with chunks of 8 / 16 levels, 512^3: lone source 7.20 / 6.87, 2 sources 8.11 / 7.15, 4: 10.57 / 9.72,
    // 8 (unpaired): 16.36 / 15.24; 256^3: 1 source 3.29 / 3.15, 2: 3.69 / 3.30, 4: 4.28 / 3.55, 8: 4.49 / 4.04 (chunks of 4: 11.99 /
    // 4.96 for the lone source; PAIRS with chunks of 16: 48 ms instead of 17 for 8 sources, 22 ms with two workgroups per CU and no
    // spills).  fp64: the lone source 8.08 / 7.39 (256^3), 13.03 / 11.40 (384^3), 2 sources 9.01 / 7.62, 4: 10.39 / 9.12, but 8 sources
    // 12.0 / 12.3 and 36.0 / 43.9 (384^3): up to four.  Same partial order, same results, same exact skipping (a chunk is the unit
    // that is skipped: twice as coarse).
    // The WENO stage likewise where it is bound by its chains: 256^3 fp32 1 source 380.6 / 318.3 ms per solve (46 WENO iterations),
    // 2 sources 397 / 371, but 4: 501 / 564, 8: 761 / 981 (bound by its arithmetic there, and the longer chunk costs it registers);
    // fp64 1 source 663.5 / 536.7, 2 sources 757 / 589.  profiles/r05/experiment_chunk_length.txt
    if (f.dim == 3 && f.C0 == 8 && f.NS == 1 && p.XS) {
        const int below = p.H == 2 ? t.weno_c16_below : f.f32 ? std::numeric_limits<int>::max() : t.f64_c16_below;
        // (the tolerance-grade kernels of one field per workgroup exist with chunks of 16 levels only)
        if ((f.opt.lone_chunk == 16 || fast) && f.batch < below) p.chunk = 16;
    }
    // tolerance-grade arithmetic: the AR = 1 instantiation of the same kernel (fsm_fast.hip).  Fields kept in pairs have one in the
    // first-order 3-D sweeps only; the WENO stage and the 2-D sweeps of such a grid (TTCR_FSM_PAIR = 1: tuning only) keep the exact kernels
    p.AR = fast && p.XS && (f.NS == 1 || (p.H == 1 && f.dim == 3));
    // first-order 3-D kernels: workgroups take units until the tickets run out -- no more of them than can be resident
    // (8 per CU is more than any instantiation fits; the surplus finds the ticket counter exhausted).  The others (and
    // TTCR_FSM_WGS=0, tuning): one workgroup per unit.  (fsm_looped, fsm_kernels.h)
    const bool looped = f.dim == 3 && p.H == 1;
    const size_t wg_cap = (looped && t.persist_wgs > 0) ? (size_t)t.persist_wgs : ~(size_t)0;
    const size_t units = (size_t)f.n_patches * f.batch * (p.XS ? ndir : 1);
    p.wgs = (unsigned)std::min(units, wg_cap);
    p.launches = p.XS ? 1 : ndir;
    if (!p.XS) { p.tickets = SweepPlan::PER_SWEEP; return p; }
    // whole iteration in one launch: tickets direction-major, sweeps overlap at their ends
    p.tickets = f.batch < t.time_order_below ? SweepPlan::XS_BY_TIME : SweepPlan::XS_BY_SWEEP;
    // (the occupancy cap of the lone source and the upwind counters sampled one chunk ahead (PRE) were tuned for chunks of 8 levels: on
    // first-order chunks of 16 they cost -- lone source 512^3 6.89 -> 6.68 ms per sweep-iteration without both, 256^3 3.19 -> 3.07, fp64
    // 256^3 7.35 -> 7.11; batches without PRE: 512^3 x 2 / 4 sources 7.21 -> 7.09 / 9.69 -> 9.64, 256^3 x 2 / 4 / 8 3.30 -> 3.15 /
    // 3.57 -> 3.47 / 4.04 -> 3.97)
    if (p.chunk == 16 && p.H == 1 && f.dim == 3) return p;
    p.dyn_lds = (f.dim == 3 && f.stage == 0 && f.batch < t.xs_lds_below) ? t.xs_lds_bytes : 0;
    p.PRE = f.dim == 2 || f.batch >= t.pre_min || p.dyn_lds > 0;   // counters sampled one chunk ahead
    return p;
}

// The instantiation's name as the compiler spells it: what ttcr_fsm_last_kernel reports and the tests compare.
inline std::string fsm_sweep_name(const SweepPlan& p) {
    const auto b = [](bool v) { return v ? "true" : "false"; };
    char nm[160];
    if (!p.persistent)
        std::snprintf(nm, sizeof nm, "fsm_sweep_tile<%s,%d,%d,%d,%s>", p.f32 ? "float" : "double", p.PJ, p.PK, p.BL, b(p.dim == 3));
    else
        std::snprintf(nm, sizeof nm, "fsm_sweep_persistent<%s,%d,%d,%d,%s,%s,%d,%d,%s,%s%s>", p.f32 ? "float" : "double", p.PJ, p.PK, p.chunk,
                      b(p.dim == 3), b(p.skip != 0), p.H, p.NS, b(p.XS), b(p.PRE), p.AR ? ",1" : "");
    return nm;
}
