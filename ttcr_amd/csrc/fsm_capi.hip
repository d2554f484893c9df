// ttcr_amd/csrc/fsm_capi.hip -- host side of the MI355X FSM solver + the C ABI of
// include/ttcr_amd.h.  Mirrors the *interface* of the reference's Grid3D/Grid2D FSM leaves
// (ttcr/Grid3Drnfs.h, Grid3Drcfs.h, Grid2Drnfs.h, Grid2Drcfs.h) -- constructor arguments,
// setSlowness/getTT/raytrace semantics, error messages -- on top of the kernels in
// fsm_kernels.h.  There is no CPU fallback: without a HIP device every call fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ttcr_amd.h"
#include "fsm_kernels.h"
#include "fsm_fast_api.h"
#include "fsm_tape_api.h"
#include "fsm_adjoint_api.h"
#include "fsm_unit_order.h"
#include "fsm_chunk_dirty.h"

namespace ttcr_amd {

static thread_local std::string g_last_error;

struct ValueError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct DeviceError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct Unsupported : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                          \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            std::ostringstream _m;                                                               \
            _m << "HIP error " << hipGetErrorString(_e) << " at " << __FILE__ << ":" << __LINE__ \
               << " (" #expr ")";                                                                \
            throw DeviceError(_m.str());                                                         \
        }                                                                                        \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    size_t guard = 0;   // elements allocated in front of p and behind p + n (readable, never meaningful)
    void reserve(size_t m, size_t guard_ = 0) {
        if (m <= n && guard_ <= guard) return;
        release();
        char* raw = nullptr;
        HIP_CHECK(hipMalloc((void**)&raw, (m + 2 * guard_) * sizeof(T)));
        guard = guard_;
        p = (T*)raw + guard;
        n = m;
    }
    void release() {
        if (p) (void)hipFree((void*)(p - guard));
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

struct Timing {
    double sweep_ms = 0, total_ms = 0;
    long long launches = 0, node_updates = 0, evaluated_updates = 0;
    int iterations = 0, n_sources = 0;
};

// what the model vector of a field tape holds, as the entry that makes the tape names it
enum TapeWrt { WRT_NODES = 0, WRT_CELLS = 1, WRT_MODEL = 2 };

class GridBase {
   public:
    virtual ~GridBase() {}
    virtual void set_slowness(const void* s, size_t n, bool on_device, bool c_order = false) = 0;
    virtual void get_slowness(void* out, size_t n) = 0;
    // explicit_slots (optional): source n is solved in slot explicit_slots[n] (ascending, distinct) -- the combined
    // single-source calls of several host threads; otherwise the sources are block-distributed like get_blk_size
    // force_rays: keep the rays of this call whatever the "return_rays" option says
    virtual void raytrace_multi(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                const void* rx, void* tt_out, int forced_slot, const int* explicit_slots = nullptr,
                                bool force_rays = false) = 0;
    // one source in `slot`, traveltimes AND rays, the rays kept per slot (raytrace overloads with r_data called by several
    // host threads at once, ttcr/Grid3D.h:855-905: every thread finds its own rays whatever the others do meanwhile)
    virtual void raytrace_rays(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out) = 0;
    virtual void slot_rays_size(int slot, size_t* n_rays, size_t* n_points) const = 0;
    virtual void get_slot_rays(int slot, long long* offsets, void* pts) const = 0;
    // the same with the entries of the matrix M per receiver (m_data overloads), kept per slot like the rays
    // both: the overload that keeps the rays as well (its terms differ, see fsm_raypath3d_m)
    virtual void raytrace_m(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out, bool both) = 0;
    virtual void slot_m_size(int slot, size_t* n_rows, size_t* nnz) const = 0;
    virtual void get_slot_m(int slot, long long* row_off, long long* j, void* v) const = 0;
    // every source of a call at once (batched solves, then the walks); one CSR over all receiver rows of the call
    virtual void raytrace_multi_m(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx,
                                  void* tt_out, bool both) = 0;
    virtual void multi_m_size(size_t* n_rows, size_t* nnz) const = 0;
    virtual void get_multi_m(long long* row_off, long long* j, void* v) const = 0;
    // the same matrix (without rays) kept on the device: the (row, node, value) entries of every receiver row of the call, rows in call
    // order, nodes ascending within a row, on `device` (the M tape, ttcr_fsm_raytrace_multi_tape)
    virtual void raytrace_multi_tape(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx,
                                     void* tt_out, TapeRows& out) = 0;
    // the field tape (ttcr_fsm_raytrace_multi_adjoint): the batched solves of raytrace_multi with interpolated receiver traveltimes
    // (whatever tt_from_rp says); after each batch every event's field, frozen nodes and receiver stencils go to `sink`
    virtual void raytrace_multi_adjoint(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx,
                                        void* tt_out, AdjSink& sink) = 0;
    // node counts and spacing of a grid the adjoint is defined for; Unsupported (with the reason) for every other grid.  wrt names the
    // entry the call came through (TapeWrt): the cell entry takes cell grids only (ValueError on a node grid), the node entry keeps
    // refusing cell grids (Unsupported), the model entries take node grids only (ValueError on a cell grid)
    virtual void adjoint_geometry(int* nn3, double* spacing, TapeWrt wrt) const = 0;
    AdjSink* adj_sink = nullptr;          // set for the duration of such a call
    std::vector<int> adj_src, adj_row;    // a replica of a multi-device grid: event and first row, in the call, of each source of ITS call
    // the raytrace overloads with l_data (2-D cell grids): ray-projection matrix L, one CSR row per receiver
    virtual void raytrace_l(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out, bool with_rays) = 0;
    virtual void slot_l_size(int slot, size_t* n_rows, size_t* nnz) const = 0;
    virtual void get_slot_l(int slot, long long* row_off, long long* cell, void* v) const = 0;
    virtual void raytrace_multi_l(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx,
                                  void* tt_out, bool with_rays) = 0;
    virtual void multi_l_size(size_t* n_rows, size_t* nnz) const = 0;
    virtual void get_multi_l(long long* row_off, long long* cell, void* v) const = 0;
    virtual void validate_points(int n_tx, const void* tx, int n_rx, const void* rx) = 0;   // throws like raytrace would
    // single-source calls that arrive together (ttcrpy's thread pool: nt host threads, one slot each) are solved together
    struct Request {
        int slot, n_tx, n_rx;
        const void *tx, *t0, *rx;
        void* tt;
        int status = TTCR_OK;
        std::string err;
        bool done = false;
    };
    std::mutex q_mu;
    std::condition_variable q_cv;
    std::vector<Request*> queue;
    bool leader_active = false;
    bool had_company = false;      // two calls have been seen on this handle at the same time (guarded by q_mu)
    std::atomic<int> combine_window_us{200};   // how long a call waits for company (option "combine_window_us"; 0: never)
    size_t elem_size = 4;
    virtual void get_tt(int slot, void* out, size_t n) = 0;
    virtual void* tt_device(int slot) = 0;                      // contiguous copy of the field (see ttcr_amd.h)
    virtual void* tt_device_view(int slot, size_t* stride) = 0;  // the field where it lies + its element stride
    std::mutex mu;  // one call at a time per handle: stream, graph capture, pinned and scratch buffers are shared
    virtual void interp(int slot, int n, const void* pts, void* out) = 0;
    virtual void compute_slowness(int n, const void* pts, bool translated, void* out) = 0;
    virtual void rays_size(size_t* n_rays, size_t* n_points) const = 0;
    virtual void get_rays(long long* offsets, void* pts) const = 0;
    int dim = 3, dtype = 0, n_slots = 1, device = 0;
    size_t n_nodes = 0, n_cells = 0;
    std::vector<int> niter, niterw;
    // Where the field of (logical) slot s lives: phys[s].  A slot is what the caller's thread number names; the batch driver
    // may give the sources of a call to other physical slots than the block distribution names (it pairs sources that lie
    // close to each other, see raytrace_multi) and records here where each one went.  Always a permutation; everything
    // inside the grid (solve_batch, the per-slot device arrays, niter, change_hist) is indexed by PHYSICAL slot, every entry
    // point that takes a slot translates.
    std::vector<int> phys;
    int P(int slot) const { return phys.empty() ? slot : phys[slot]; }
    int stopping_shortcuts = 3; // option "stopping_shortcuts", bits: 1 the passes of the stopping rule over a field and its snapshot read only the bricks
                                // the sweep kernels stamped as changed, where such stamps are kept; 2 the ordered sum is left out where bounds on
                                // it already put it on one side of eps * N (GridT::decide_go_on).  0: whole fields, every sum (tests, bisecting)
    int stopping_rule = 1;      // option "stopping_rule": 1 (default) the reference's sequential T1 sum decides wherever it could differ from the
                                // fp64 sum of decreases, 0 the fp64 sum alone (default: the sequential sum is 1.3e8 dependent additions
                                // per 512^3 field and iteration it is asked for -- 11.7 s instead of 0.32 s for the heterogeneous bench leg)
    long long reference_sums = 0, reference_sums_missed = 0;   // decisions taken with the reference's sum / that would have needed a snapshot
    long long refsum_rounds = 0;                               // rounds of the parallel form of that sum (fsm_refsum_*)
    virtual void stopping_stats(long long* sums, long long* missed, long long* rounds) const {
        if (sums) *sums = reference_sums;
        if (missed) *missed = reference_sums_missed;
        if (rounds) *rounds = refsum_rounds;
    }
    // the reference's `change` of two fields given on the host (n_nodes values each, node order): sum of abs(times[n] - field[n]) in T1,
    // in node order; parallel: the exact parallel form, else the one-chain kernel (tests compare the two)
    virtual void reference_change_host(const void* times, const void* field, bool parallel, void* out) = 0;
    int pair_by_distance = 1;   // option "pair_sources" (0: every source in the slot the block distribution names)
    virtual void set_pair_layout(int) {}
    virtual long long prefill_inline_count() const { return 0; }   // calls whose first sweep launch filled the spare set (ttcr_fsm_prefill_inline_fills)
    virtual long long prefill_swap_count() const { return 0; }   // calls that took fields initialised on the side stream (ttcr_fsm_prefill_swaps)
    int lone_chunk = 16;   // option "lone_chunk" / TTCR_FSM_LONE_CHUNK: levels per chunk of the fp32 first-order 3-D kernels with one field per workgroup (8 or 16)
    int arith = 0;      // option "arith" / TTCR_FSM_ARITH: 0 (default) the reference's arithmetic, results bit-identical to it; 1 tolerance-grade
                        // fp32 local solvers in the first-order sweeps of fp32 grids without the WENO stage (update3_fast / update2_fast,
                        // fsm_kernels.h): within north_star's 1e-5 s RMS of the reference, NOT bit-identical; 2: the WENO stage too
                        // (weno_axis_fast; outside that bound, see fsm_fast_arith); whole-iteration launches only
    int prefill = -1;   // option "prefill" / TTCR_FSM_PREFILL: a second set of traveltime fields, re-initialised on a side stream while a
                        // solve runs, which the next call that restarts EVERY slot swaps in instead of filling (GridT::solve_batch);
                        // 1 on, 0 off, -1 (default): on when the fields take at least 64 MiB and twice that is at most half the device memory
    int prefill_inline = -1;   // option "prefill_inline": the spare set is filled by the units of the call's first whole-iteration sweep launch
                               // instead of on the side stream (GridT::inline_fill_now); 1 on, 0 off, -1 (default): see there
    // L1 change of every sweep-iteration of the last solve of a slot (what the stopping rule compared with eps * N), first-
    // order stage then WENO stage
    std::vector<std::vector<double>> change_hist, change_histw;
    // ... and the reference's own sum (sequential, in T1) for the iterations that were decided with it (option stopping_rule; NaN: the others)
    std::vector<std::vector<double>> ref_hist, ref_histw;
    virtual void get_reference_changes(int slot, double* first, int n_first, double* wen, int n_weno) const {
        if (slot < 0 || slot >= n_slots) throw ValueError("Thread number is larger than number of threads");
        slot = P(slot);
        for (int q = 0; q < n_first; ++q) first[q] = (!ref_hist.empty() && q < (int)ref_hist[slot].size()) ? ref_hist[slot][q] : std::nan("");
        for (int q = 0; q < n_weno; ++q) wen[q] = (!ref_histw.empty() && q < (int)ref_histw[slot].size()) ? ref_histw[slot][q] : std::nan("");
    }
    virtual void get_changes(int slot, double* first, int n_first, double* wen, int n_weno) const {
        if (slot < 0 || slot >= n_slots) throw ValueError("Thread number is larger than number of threads");
        slot = P(slot);
        for (int q = 0; q < n_first; ++q) first[q] = (!change_hist.empty() && q < (int)change_hist[slot].size()) ? change_hist[slot][q] : 0.0;
        for (int q = 0; q < n_weno; ++q) wen[q] = (!change_histw.empty() && q < (int)change_histw[slot].size()) ? change_histw[slot][q] : 0.0;
    }
    bool weno = false;
    bool sweep45_strips = false;  // force the strip kernel of sweep45 (env TTCR_FSM_SWEEP45=strips; tests)
    bool rotated = false;  // 2-D rotated_template: sweep45 after every first-order sweep (ttcr/Grid2Drnfs.h:277-286)
    int ttrp = 0, interp_vel = 0;  // traveltime from raypath (ttcr/Grid3D.h:493-496), processVel
    std::atomic<int> return_rays{0};   // raytrace overloads with r_data (ttcr/Grid3D.h:546-586): rays kept for get_rays
    int fixed_iters = 0, max_batch = 0, use_graph = 1;
    int skip = -1; // persistent kernel: 1 = skip chunks whose read set did not change (exact); 0 = evaluate
                   // every chunk; -1 (default) = on for a lone source with the WENO stage (256^3: 427 -> 368 ms), off otherwise
    int mode = 2;  // 2: persistent kernel, one launch per sweep-iteration, sweeps overlap (default);
                   // 1: persistent kernel, one launch per sweep; 0: one launch per tile wavefront
    Timing timing;
    std::string last_kernel;   // instantiation of the sweep kernel the last solve launched (ttcr_fsm_last_kernel)
    virtual std::string kernel_name() const { return last_kernel; }
    long walk_step_limit = 1000000;   // steps after which a ray walk is declared endless (the oracle uses the same number)
    long walk_records = 0;   // option "walk_records": records per row of the recording ray walks (rays, compute_M, the M tape, compute_L) in place
                             // of eight per node of the grid's extent (0, default); a walk that needs more is walked again alone with room
    long walk_room(long extent) const { return std::min<long>(walk_step_limit, walk_records > 0 ? walk_records : extent); }
    // ttcr_fsm_set_option (a multi-device grid forwards it to its replicas)
    virtual void apply_option(const std::string& k, double value) {
        if (k == "fixed_iters") fixed_iters = (int)value;
        else if (k == "max_batch") max_batch = (int)value;
        else if (k == "use_graph") use_graph = (int)value;
        else if (k == "combine_window_us") combine_window_us = (int)value;
        else if (k == "mode") mode = (int)value;
        else if (k == "skip") skip = (int)value;
        else if (k == "tt_from_rp") ttrp = value != 0;
        else if (k == "interp_vel") interp_vel = value != 0;
        else if (k == "return_rays") return_rays = value != 0;
        else if (k == "pair_sources") pair_by_distance = value != 0;
        else if (k == "pair_layout") {
            if (value != -1 && value != 0 && value != 1) throw ValueError("option 'pair_layout': -1 (default), 0 or 1");
            set_pair_layout((int)value);
        }
        else if (k == "stopping_rule") stopping_rule = (int)value;
        else if (k == "stopping_shortcuts") { if (value < 0 || value > 3 || value != (double)(int)value) throw ValueError("option stopping_shortcuts: 0 ... 3"); stopping_shortcuts = (int)value; }
        else if (k == "prefill") {
            if (value != -1 && value != 0 && value != 1) throw ValueError("option 'prefill': -1 (default), 0 or 1");
            prefill = (int)value;
        } else if (k == "prefill_inline") {
            if (value != -1 && value != 0 && value != 1) throw ValueError("option 'prefill_inline': -1 (default), 0 or 1");
            prefill_inline = (int)value;
        } else if (k == "lone_chunk") {
            if (value != 8 && value != 16) throw ValueError("option 'lone_chunk': 8 or 16");
            lone_chunk = (int)value;
        }
        else if (k == "arith") {
            if (value != 0 && value != 1 && value != 2)
                throw ValueError("option 'arith': 0 (the reference's arithmetic), 1 (tolerance-grade fp32 where it stays within 1e-5 s RMS) or 2 (the WENO stage as well)");
            arith = (int)value;
        }
        else if (k == "walk_records") {
            if (value != 0 && !(value >= 1 && value <= (double)walk_step_limit && value == (double)(long)value))
                throw ValueError("option 'walk_records': 0 (default) or a whole number from 1 to the step limit of a walk");
            walk_records = (long)value;
        }
        else throw ValueError("unknown option '" + k + "'");
    }
    virtual void get_niter(int slot, int* it, int* itw) const {
        if (slot < 0 || slot >= n_slots) throw ValueError("Thread number is larger than number of threads");
        if (it) *it = niter[P(slot)];
        if (itw) *itw = niterw[P(slot)];
    }
};

// Every exact sweep kernel there is (T, DIM, H, NS, chunk[, PRE]); the tolerance-grade ones: fsm_fast.hip
template <typename T>
using ExactSweepKernels = SweepKernels<
    // 3-D WENO stage: one field per workgroup on chunks of 16 levels (whole-iteration launch), pairs and one field on chunks of 4 and of 8
    WholeIteration<T, 3, 2, 1, 16>, EveryLaunch<T, 3, 2, 2, 4>, EveryLaunch<T, 3, 2, 1, 4>, EveryLaunch<T, 3, 2, 2, ChunkCfg<T, 3>::C>,
    EveryLaunch<T, 3, 2, 1, ChunkCfg<T, 3>::C>,
    // 2-D WENO stage
    EveryLaunch<T, 2, 2, 2, ChunkCfg<T, 2>::C>, EveryLaunch<T, 2, 2, 1, ChunkCfg<T, 2>::C>,
    // first-order 3-D sweeps: one field on chunks of 16 (whole-iteration launch, no PRE), pairs and one field on chunks of 8
    WholeIterationPre<T, 3, 1, 1, 16, false>, EveryLaunch<T, 3, 1, 2, ChunkCfg<T, 3>::C>, EveryLaunch<T, 3, 1, 1, ChunkCfg<T, 3>::C>,
    // first-order 2-D sweeps
    EveryLaunch<T, 2, 1, 2, ChunkCfg<T, 2>::C>, EveryLaunch<T, 2, 1, 1, ChunkCfg<T, 2>::C>>;
// Whether the library holds the kernel a plan names (fsm_sweep_tile exists for every grid), and its launch.
template <typename T>
static bool sweep_kernel_exists(const SweepPlan& p) {
    if (!p.persistent) return true;
    if (p.AR) return std::is_same<T, float>::value && fsm_fast_sweep_exists(p);
    return ExactSweepKernels<T>::has(p);
}
template <typename T>
static void launch_sweep_kernel(const SweepPlan& p, const PersistArgs<T>& pa, hipStream_t stream) {
    if constexpr (std::is_same<T, float>::value)
        if (p.AR) { fsm_fast_sweep(p, pa, stream); return; }
    ExactSweepKernels<T>::run(p, pa, stream);
}

template <typename T>
class GridT : public GridBase {
   public:
    // reference geometry, all in T like the reference members (ttcr/Grid3Drn.h:67-78)
    uint32_t ncx, ncy, ncz;  // cells; 2-D: ncy = 0
    T dx, dz, xmin, ymin, zmin, xmax, ymax, zmax, ox = 0, oy = 0, oz = 0;
    T epsilon;
    int nitermax;
    bool cell, translate;
    bool have_slowness = false;

    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<T> d_s, d_cells, d_tt, d_rx, d_out;
    // Re-initialisation off the path of a call (reinit, ttcr/Grid3Drnfs.h:92-94: T = max() everywhere -- 32 GB of stores for 64 fields
    // of 512^3 nodes, 6.8 ms at the write bandwidth of the device).  d_tt_alt is a second set of fields: while a solve that restarted
    // every slot runs in d_tt, a low-priority side stream fills d_tt_alt; the next call that restarts every slot swaps the two and
    // finds its fields initialised.  A call that restarts only some slots fills them in place as before (the other slots keep their
    // fields, as the reference's per-thread grids do).  Nothing outside the grid sees the swap except device views, which are valid
    // "until the next raytrace call that solves a source for that slot" (include/ttcr_amd.h).
    DevBuf<T> d_tt_alt;
    bool alt_filled = false;        // a fill of d_tt_alt has been issued on fill_stream (ev_fill marks its end)
    hipStream_t fill_stream = nullptr;
    hipEvent_t ev_fill = nullptr;
    long long prefill_swaps = 0;    // calls that found their fields initialised
    long long prefill_swap_count() const override { return prefill_swaps; }
    long long prefill_inline_fills = 0;   // calls whose first sweep launch filled the spare set
    long long prefill_inline_count() const override { return prefill_inline_fills; }
    void set_pair_layout(int v) override { pair_layout = v; }
    DevBuf<int> d_rslot;
    DevBuf<RaySrc> d_rdesc;
    SweepTuning tune;   // thresholds of the kernel choice (fsm_sweep_plan.h), read from the environment when the grid is created
    DevBuf<T> d_gather;      // scratch for de-interleaving one field
    DevBuf<T> d_rsrc, d_rt0;  // source points / origin times of the source whose rays are traced
    DevBuf<int> d_rstat;
    DevBuf<T> d_ssh;         // sheared copies of the node slowness, one per direction family
    size_t ssh_stride = 0;   // elements per copy: NK planes of shear_plane(geom) elements
    DevBuf<uint32_t> d_mask;
    DevBuf<int> d_bbox, d_slots, d_lmask;
    int* h_lmask = nullptr;  // pinned
    DevBuf<uint32_t> d_tiles;            // per launch w: the patches that have nodes in it
    std::vector<int> tile_off, tile_cnt;  // offsets / counts into d_tiles
    DevBuf<double> d_change;
    DevBuf<unsigned long long> d_prof;  // TTCR_FSM_PROF=1 debug phase timers
    size_t prof_words = 0;
    DevBuf<uint32_t> d_order;  // persistent kernel: patches in ticket order (anti-diagonal major)
    DevBuf<uint32_t> d_order_xs[2][2];  // whole-iteration launch, [stage: first order / WENO][0: sweep by sweep, 1: by expected start time]
    DevBuf<int> d_sync;        // persistent kernel: ticket, abort flag, per (source, patch) progress
    int n_patches = 0;
    int* h_abort = nullptr;    // pinned
    DevBuf<int> d_stamp;       // dirty-brick stamps [n_slots][nbf*nbj*nbk]
    DevBuf<unsigned> d_cdirty;   // first-order 3-D SKIP kernels: chunk-shaped dirty bits [slot group][dir][patch][cdirty_wpu] (fsm_chunk_dirty.h)
    DevBuf<unsigned long long> d_cmap;   // SKIP kernels: per-chunk edge-change flags of every unit of a launch [dir][entry][patch][2][cmap_words]
    int cmap_words = 1;
    DevBuf<unsigned long long> d_sw;   // SKIP kernels: per (global sweep, slot group) units finished | units that changed a node
    int sw_sweeps = 0;
    DevBuf<int> d_iter;        // current iteration index (read by the captured kernels)
    DevBuf<unsigned long long> d_evals;  // [n_slots] node updates actually evaluated
    int* h_iter = nullptr;     // pinned: [0] iteration index, [1] launch epoch
    unsigned launch_epoch = 1;  // number of the next sweep launch of this grid (0: never -- what zeroed memory reads as)
    bool sync_clean = true;     // the last solve ended normally (else the synchronisation words are wiped before the next one)
    size_t sync_words = 0;
    unsigned long long* h_evals = nullptr;  // pinned
    int nbf = 0, nbj = 0, nbk = 0;
    size_t n_bricks = 0;
    DevBuf<InitPoint<T>> d_pts;
    double* h_change = nullptr;  // pinned
    int* h_slots = nullptr;      // pinned
    size_t mask_words = 0;
    SweepGeom geom;
    int n_launch = 0;  // launches per sweep direction
    // one captured launch sequence per stage (first-order / WENO3)
    hipGraph_t graphs[2] = {nullptr, nullptr};
    hipGraphExec_t graph_execs[2] = {nullptr, nullptr};
    SweepPlan graph_plans[2];   // what each holds (batch -1: no longer valid)

    GridT(int dim_, bool cell_, uint32_t nx, uint32_t ny, uint32_t nz, double ddx, double ddz, double minx,
          double miny, double minz, double eps, int maxit, int nslots, bool translate_, int dev, bool weno_) {
        dim = dim_;
        weno = weno_;
        dtype = sizeof(T) == 4 ? TTCR_F32 : TTCR_F64;
        elem_size = sizeof(T);
        cell = cell_;
        translate = translate_;
        ncx = nx; ncy = ny; ncz = nz;
        dx = (T)ddx;
        dz = (T)ddz;
        xmin = (T)minx; ymin = (T)miny; zmin = (T)minz;
        // xmax(minx+nx*ddx) etc. in T arithmetic (ttcr/Grid3Drn.h:73, ttcr/Grid2Drn.h:62)
        xmax = xmin + (T)nx * dx;
        if (dim == 3) {
            ymax = ymin + (T)ny * dx;
            zmax = zmin + (T)nz * dx;
        } else {
            ymax = ymin;
            zmax = zmin + (T)nz * dz;
        }
        if (translate) {  // buildGridNodes, ttcr/Grid3Drn.h:362-372
            ox = xmin; oy = ymin; oz = zmin;
            xmax -= xmin; ymax -= ymin; zmax -= zmin;
            xmin = 0; ymin = 0; zmin = 0;
        }
        n_nodes = dim == 3 ? (size_t)(nx + 1) * (ny + 1) * (nz + 1) : (size_t)(nx + 1) * (nz + 1);
        n_cells = dim == 3 ? (size_t)nx * ny * nz : (size_t)nx * nz;
        if (n_nodes >= (1ull << 32)) throw ValueError("grid too large: node index must fit uint32 (reference T2)");
        epsilon = (T)eps;
        epsilon *= (T)n_nodes;  // ttcr/Grid3Drnfs.h:49
        nitermax = maxit;
        n_slots = nslots;
        niter.assign(n_slots, 0);
        niterw.assign(n_slots, 0);
        phys.resize(n_slots);
        for (int q = 0; q < n_slots; ++q) phys[q] = q;
        max_batch = n_slots;
        device = dev;
        HIP_CHECK(hipSetDevice(device));
        {
            int cus = 0;
            HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
            tune = fsm_sweep_tuning(8 * std::max(cus, 1));
            const SweepOptions o = fsm_sweep_options();
            mode = o.mode; skip = o.skip; lone_chunk = o.lone_chunk; arith = o.arith;
        }
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreate(&ev0));
        HIP_CHECK(hipEventCreate(&ev1));
        d_s.reserve(n_nodes, 64);
        {   // source pairs for the first-order 3-D solver only (fsm_pair_layout)
            const long long patches = dim == 3 ? (long long)((ny + 1 + TileCfg<T, 3>::PJ - 1) / TileCfg<T, 3>::PJ) * ((nz + 1 + TileCfg<T, 3>::PK - 1) / TileCfg<T, 3>::PK) : 0;
            NS = fsm_pair_layout(tune, dim, weno, n_slots, patches, &ns_window);
        }
        d_tt.reserve(n_nodes * tt_fields(), 64);   // (room for either layout)
        mask_words = (n_nodes + 31) / 32;
        d_mask.reserve(mask_words * (size_t)n_slots);
        d_bbox.reserve(6 * (size_t)n_slots);
        d_slots.reserve(n_slots);
        d_lmask.reserve(n_slots);
        HIP_CHECK(hipHostMalloc((void**)&h_lmask, sizeof(int) * n_slots));
        d_change.reserve(n_slots);
        if (std::getenv("TTCR_FSM_PROF")) {   // FSM_ENABLE_PROF builds: 8 phase sums + a 4-word trace entry per work unit
            prof_words = 8 + 4 * (size_t)(1 << 20);
            d_prof.reserve(prof_words);
            HIP_CHECK(hipMemset(d_prof.p, 0, prof_words * sizeof(unsigned long long)));
        }
        HIP_CHECK(hipHostMalloc((void**)&h_change, sizeof(double) * n_slots));
        HIP_CHECK(hipHostMalloc((void**)&h_slots, sizeof(int) * n_slots));
        HIP_CHECK(hipHostMalloc((void**)&h_abort, sizeof(int)));
        *h_abort = 0;
        HIP_CHECK(hipHostMalloc((void**)&h_iter, 2 * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_evals, sizeof(unsigned long long) * n_slots));
        HIP_CHECK(hipMemsetAsync(d_tt.p, 0, n_nodes * tt_fields() * sizeof(T), stream));

        if (dim == 3) {
            using C = TileCfg<T, 3>;
            geom.NF = nx + 1; geom.NJ = ny + 1; geom.NK = nz + 1;
            geom.npj = (geom.NJ + C::PJ - 1) / C::PJ;
            geom.npk = (geom.NK + C::PK - 1) / C::PK;
            n_launch = fsm_tile_launches(geom.NF, geom.NJ, geom.NK, geom.npj, geom.npk, C::BL);
        } else {  // F = z (fastest), J = x
            using C = TileCfg<T, 2>;
            geom.NF = nz + 1; geom.NJ = nx + 1; geom.NK = 1;
            geom.npj = (geom.NJ + C::PJ - 1) / C::PJ;
            geom.npk = 1;
            n_launch = fsm_tile_launches(geom.NF, geom.NJ, geom.NK, geom.npj, geom.npk, C::BL);
        }
        geom.n_nodes = (uint32_t)n_nodes;
        geom.M = (std::max(geom.NF, geom.NJ) + 1) & ~1;
        geom.MP = geom.M + FSM_XPAD;
        geom.SR = dim == 3 ? ((geom.NJ + 15) / 16) * 32 : 0;   // 2-D: plain rows (fsm_kernels.h, shear_index)
        ssh_stride = (size_t)geom.NK * shear_plane(geom);
        // (the sweep kernels address a thread's plane of a copy with a 32-bit byte offset from the plane of its patch's first row)
        if ((double)(dim == 3 ? 16 : 1) * (double)shear_plane(geom) * sizeof(T) >= 4294967296.0)
            throw ValueError("grid too large for the slowness offsets of the sweep kernel (16 planes of max(nx, ny) x ny nodes must stay below 4 GiB)");
        d_ssh.reserve(ssh_stride * (dim == 3 ? 4 : 2));
        HIP_CHECK(hipMemsetAsync(d_ssh.p, 0, ssh_stride * (dim == 3 ? 4 : 2) * sizeof(T), stream));   // (entries without a node are read, never used)
        if (dim == 3) build_tile_lists(TileCfg<T, 3>::PJ, TileCfg<T, 3>::PK, TileCfg<T, 3>::BL);
        else build_tile_lists(TileCfg<T, 2>::PJ, TileCfg<T, 2>::PK, TileCfg<T, 2>::BL);
        build_persistent_lists();
        nbf = (geom.NF + FSM_BRICK - 1) / FSM_BRICK;
        nbj = (geom.NJ + FSM_BRICK - 1) / FSM_BRICK;
        nbk = (geom.NK + FSM_BRICK - 1) / FSM_BRICK;
        n_bricks = (size_t)nbf * nbj * nbk;
        d_stamp.reserve(n_bricks * n_slots);  // one set per slot group is used
        {
            // change maps of the SKIP kernels: one bit per chunk and edge; a unit has at most (NF + PJ + PK) / C + 2 chunks
            // (the shortest chunks any instantiation uses are 4 levels long), and reads a little past the end of its
            // upwind units' maps
            const int PJ = dim == 3 ? TileCfg<T, 3>::PJ : TileCfg<T, 2>::PJ, PK = dim == 3 ? TileCfg<T, 3>::PK : 1;
            const int max_chunks = (geom.NF + 2 * (PJ + PK)) / 4 + 4;
            cmap_words = max_chunks / 32 + 1;
            d_cmap.reserve((size_t)n_patches * n_slots * (dim == 3 ? 8 : 4) * 2 * cmap_words);
            HIP_CHECK(hipMemset(d_cmap.p, 0, (size_t)n_patches * n_slots * (dim == 3 ? 8 : 4) * 2 * cmap_words * sizeof(unsigned long long)));
            cdirty_wpu = fsm_cdirty_wpu(geom.NF, PJ, PK);
            if (dim == 3) d_cdirty.reserve(cdirty_words());   // (one set per slot group, at most n_slots of them; zeroed by every solve)
            // whole-sweep tallies: one entry per sweep of a solve (both stages); solves with more sweeps simply stop using them
            sw_sweeps = (dim == 3 ? 8 : 4) * (2 * std::min(nitermax, 256) + 2);
            d_sw.reserve((size_t)sw_sweeps * n_slots);   // (one entry per slot group: at most n_slots of them, whichever the layout)
        }
        d_iter.reserve(2);
        d_evals.reserve(n_slots);
        if (dim == 2)   // the row-parallel sweep45 kernel keeps four rows in (dynamic) LDS
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fsm_sweep45_rows<T>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
        if (const char* e = std::getenv("TTCR_FSM_SWEEP45")) sweep45_strips = std::string(e) == "strips";
        if (const char* e = std::getenv("TTCR_FSM_RS_FIELDS")) rs_fields_max = (size_t)std::max(0, std::atoi(e));   // tests: batches of the stopping rule's sums (0: strided fields)
        if (const char* e = std::getenv("TTCR_FSM_PREFILL")) prefill = std::atoi(e);
    }

    // persistent kernel: ticket order = anti-diagonal m = TJ+TK major (a topological order of the
    // patch dependencies), progress counters per (source slot in batch, patch)
    void build_persistent_lists() {
        const std::vector<uint32_t> order = fsm_diag_order(geom.npj, geom.npk);
        n_patches = (int)order.size();
        d_order.reserve(order.size());
        HIP_CHECK(hipMemcpy(d_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        // four ticket counters, the abort word, then one progress word per (direction, slot, patch).  The kernels tag every
        // word with the launch epoch: nothing is reset between the launches of a solve (fsm_kernels.h, "launch epoch")
        sync_words = 8 + (size_t)n_patches * n_slots * (dim == 3 ? 8 : 4);
        d_sync.reserve(sync_words);
        HIP_CHECK(hipMemset(d_sync.p, 0, sync_words * sizeof(int)));
        if (geom.npj >= (1 << 14) || geom.npk >= (1 << 14)) throw ValueError("grid too large for the patch index of the sweep kernel");
        for (int st = 0; st < 2; ++st)
            for (int tm = 0; tm < 2; ++tm) {
                const std::vector<uint32_t> xs = xs_order(order, tm != 0, st == 0 ? 1 : 2);
                d_order_xs[st][tm].reserve(xs.size());
                HIP_CHECK(hipMemcpy(d_order_xs[st][tm].p, xs.data(), xs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            }
    }

    // Ticket order of the whole-iteration launch (fsm_unit_order.h, fsm_xs_order) with the tiles and chunks of this grid
    std::vector<uint32_t> xs_order(const std::vector<uint32_t>& diag_order, bool by_time, int H) const {
        const int PJ = dim == 3 ? TileCfg<T, 3>::PJ : TileCfg<T, 2>::PJ, PK = dim == 3 ? TileCfg<T, 3>::PK : 1;
        const int C = dim == 3 ? ChunkCfg<T, 3>::C : ChunkCfg<T, 2>::C;
        return fsm_xs_order(dim, geom.NF, geom.NJ, geom.NK, PJ, PK, C, H, by_time, diag_order);
    }

    // For every launch w of a sweep, the patches (TJ,TK) whose level window
    // [BL*w - (TJ+TK)*(BL-1), +BL) contains nodes.  Direction-independent (oriented indices).
    void build_tile_lists(int PJ, int PK, int BL) {
        std::vector<uint32_t> all;
        tile_off.assign(n_launch, 0);
        tile_cnt.assign(n_launch, 0);
        for (int w = 0; w < n_launch; ++w) {
            tile_off[w] = (int)all.size();
            // anti-diagonal order keeps tiles that share halo columns close in the list
            for (int m = 0; m <= geom.npj + geom.npk - 2; ++m) {
                const int L0 = BL * w - m * (BL - 1);
                for (int TK = std::max(0, m - geom.npj + 1); TK <= std::min(m, geom.npk - 1); ++TK) {
                    const int TJ = m - TK;
                    const int j0 = TJ * PJ, k0 = TK * PK;
                    const int jmaxp = std::min(j0 + PJ, geom.NJ) - 1, kmaxp = std::min(k0 + PK, geom.NK) - 1;
                    if (L0 + BL - 1 < j0 + k0 || L0 > jmaxp + kmaxp + geom.NF - 1) continue;
                    all.push_back((uint32_t)TJ | ((uint32_t)TK << 16));
                }
            }
            tile_cnt[w] = (int)all.size() - tile_off[w];
        }
        d_tiles.reserve(std::max<size_t>(all.size(), 1));
        HIP_CHECK(hipMemcpy(d_tiles.p, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }

    ~GridT() override {
        (void)hipSetDevice(device);
        for (int i = 0; i < 2; ++i) {
            if (graph_execs[i]) (void)hipGraphExecDestroy(graph_execs[i]);
            if (graphs[i]) (void)hipGraphDestroy(graphs[i]);
        }
        if (h_change) (void)hipHostFree(h_change);
        if (h_slots) (void)hipHostFree(h_slots);
        if (h_lmask) (void)hipHostFree(h_lmask);
        if (h_abort) (void)hipHostFree(h_abort);
        if (h_iter) (void)hipHostFree(h_iter);
        if (h_evals) (void)hipHostFree(h_evals);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (fill_stream) { (void)hipStreamSynchronize(fill_stream); (void)hipStreamDestroy(fill_stream); }
        if (ev_fill) (void)hipEventDestroy(ev_fill);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // ---- slowness ---------------------------------------------------------------------
    // c_order (3-D): `s` is the (nx, ny, nz) array in C order; it is uploaded as it lies and permuted to the
    // solver's x-fastest order on the device (the strided host-side flatten('F') of a 512^3 model takes 0.8 s)
    void set_slowness(const void* s, size_t n, bool on_device, bool c_order) override {
        HIP_CHECK(hipSetDevice(device));
        const size_t expect = cell ? n_cells : n_nodes;
        if (n != expect) throw std::length_error("Error: slowness vectors of incompatible size.");
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (cell) d_cells.reserve(n_cells);
        T* dst = cell ? d_cells.p : d_s.p;
        DevBuf<T> staged;
        if (c_order && dim == 3) {
            const int ax = (int)ncx + (cell ? 0 : 1), ay = (int)ncy + (cell ? 0 : 1), az = (int)ncz + (cell ? 0 : 1);
            staged.reserve(n);
            HIP_CHECK(hipMemcpyAsync(staged.p, s, n * sizeof(T), kind, stream));
            fsm_c_to_x_fastest<T><<<dim3((az + 31) / 32, (ax + 31) / 32, ay), dim3(32, 8), 0, stream>>>(staged.p, dst, ax, ay, az);
            HIP_CHECK(hipGetLastError());
        } else {
            HIP_CHECK(hipMemcpyAsync(dst, s, n * sizeof(T), kind, stream));
        }
        if (cell) {
            const int blocks = (int)std::min<size_t>((n_nodes + 255) / 256, 4096);
            if (dim == 3)
                fsm_cells_to_nodes3d<T><<<blocks, 256, 0, stream>>>(d_cells.p, d_s.p, (int)ncx, (int)ncy, (int)ncz);
            else
                fsm_cells_to_nodes2d<T><<<blocks, 256, 0, stream>>>(d_cells.p, d_s.p, (int)ncx, (int)ncz);
            HIP_CHECK(hipGetLastError());
        }
        // sheared copies (fsm_kernels.h: fsm_shear_slowness): family = F/J flips with K (3-D) or
        // J (2-D) not flipped; a direction and its opposite share one copy
        {
            const int nfam = dim == 3 ? 4 : 2;
            const dim3 grid((geom.MP + 15) / 16, (geom.NJ + 15) / 16, geom.NK);
            const bool lines = grid.y <= 65535 && grid.z <= 65535 && !std::getenv("TTCR_FSM_SHEAR_SCATTER");
            const int blocks = (int)std::min<size_t>((n_nodes + 255) / 256, 8192);
            for (int f = 0; f < nfam; ++f) {
                if (lines) fsm_shear_slowness_lines<T><<<grid, 256, 0, stream>>>(d_s.p, d_ssh.p + (size_t)f * ssh_stride, geom, f & 1, (f >> 1) & 1);
                else fsm_shear_slowness<T><<<blocks, 256, 0, stream>>>(d_s.p, d_ssh.p + (size_t)f * ssh_stride, geom, f & 1, (f >> 1) & 1);
            }
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        have_slowness = true;
    }

    void get_slowness(void* out, size_t n) override {
        HIP_CHECK(hipSetDevice(device));
        if (n != n_nodes) throw std::length_error("Error: slowness vectors of incompatible size.");
        HIP_CHECK(hipMemcpyAsync(out, d_s.p, n * sizeof(T), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    void get_tt(int slot, void* out, size_t n) override {
        HIP_CHECK(hipSetDevice(device));
        check_slot(slot);
        slot = P(slot);
        if (n != n_nodes) throw ValueError("traveltime buffer has wrong size");
        if (NS == 1) {
            HIP_CHECK(hipMemcpyAsync(out, tt_ptr(slot), n * sizeof(T), hipMemcpyDeviceToHost, stream));
        } else {
            d_gather.reserve(n_nodes);
            const int blocks = (int)std::min<size_t>((n_nodes + 255) / 256, 8192);
            fsm_gather_field<T><<<blocks, 256, 0, stream>>>(tt_ptr(slot), d_gather.p, n_nodes, NS);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(out, d_gather.p, n * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // The fields of a slot group are interleaved (T[group][node][NS]): a consumer that wants n_nodes contiguous
    // values gets a de-interleaved copy in a scratch buffer of the grid; the zero-copy view comes with its stride.
    void* tt_device(int slot) override {
        HIP_CHECK(hipSetDevice(device));
        check_slot(slot);
        slot = P(slot);
        if (NS == 1) return tt_ptr(slot);
        d_gather.reserve(n_nodes);
        const int blocks = (int)std::min<size_t>((n_nodes + 255) / 256, 8192);
        fsm_gather_field<T><<<blocks, 256, 0, stream>>>(tt_ptr(slot), d_gather.p, n_nodes, NS);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
        return d_gather.p;
    }
    void* tt_device_view(int slot, size_t* stride) override {
        check_slot(slot);
        if (stride) *stride = (size_t)NS;
        return tt_ptr(P(slot));
    }

    void check_slot(int slot) const {
        if (slot < 0 || slot >= n_slots) throw ValueError("Thread number is larger than number of threads");
    }

    // ---- points -----------------------------------------------------------------------
    int ncoord() const { return dim == 3 ? 3 : 2; }

    // Grid3Drn::checkPts (ttcr/Grid3Drn.h:771-790) / Grid2Drn::checkPts (ttcr/Grid2Drn.h:333-342)
    void check_pts(const T* p, int n) const {
        for (int m = 0; m < n; ++m) {
            if (dim == 3) {
                const T x = p[3 * m], y = p[3 * m + 1], z = p[3 * m + 2];
                if (x < xmin || x > xmax || y < ymin || y > ymax || z < zmin || z > zmax) {
                    std::ostringstream msg;
                    msg << "Error: Point (" << x << ' ' << y << ' ' << z << ") outside grid.";
                    throw std::runtime_error(msg.str());
                }
            } else {
                const T x = p[2 * m], z = p[2 * m + 1];
                if (x < xmin || x > xmax || z < zmin || z > zmax) {
                    std::ostringstream msg;
                    msg << "Error: Point (" << x << ", " << z << ") outside grid.";
                    throw std::runtime_error(msg.str());
                }
            }
        }
    }

    static T node_coord_h(T cmin, uint32_t n, T d) { return cmin + (T)n * d; }

    // first node index whose coordinate is within `small` of v (Node3Dn::operator==,
    // ttcr/Node3Dn.h:147-149, scanned in increasing order like initFSM's linear search)
    int first_match(T cmin, T d, uint32_t nn, T v) const {
        const double small = 1.e-4;
        // candidates around the nearest node; scan a window that covers every possible match
        double est = ((double)v - (double)cmin) / (double)d;
        long c = (long)std::floor(est);
        long span = (long)std::ceil(small / std::fabs((double)d)) + 2;
        long lo = std::max<long>(0, c - span), hi = std::min<long>((long)nn - 1, c + span + 1);
        for (long i = lo; i <= hi; ++i) {
            const T diff = node_coord_h(cmin, (uint32_t)i, d) - v;
            if ((double)(diff < 0 ? -diff : diff) < small) return (int)i;
        }
        return -1;
    }

    InitPoint<T> locate(const T* p, T t0) const {
        InitPoint<T> q;
        std::memset(&q, 0, sizeof(q));
        q.t0 = t0;
        if (dim == 3) {
            q.x = p[0]; q.y = p[1]; q.z = p[2];
            const int fi = first_match(xmin, dx, ncx + 1, q.x);
            const int fj = first_match(ymin, dx, ncy + 1, q.y);
            const int fk = first_match(zmin, dx, ncz + 1, q.z);
            if (fi >= 0 && fj >= 0 && fk >= 0) {
                q.on_node = 1; q.i = fi; q.j = fj; q.k = fk;
            } else {
                // Grid3Drn::getCellNo (ttcr/Grid3Drn.h:207-215) + decomposition (:3530-3534)
                const double small2 = 1.e-4 * 1.e-4;
                const T x = (double)(xmax - q.x) < small2 ? (T)((double)xmax - .5 * (double)dx) : q.x;
                const T y = (double)(ymax - q.y) < small2 ? (T)((double)ymax - .5 * (double)dx) : q.y;
                const T z = (double)(zmax - q.z) < small2 ? (T)((double)zmax - .5 * (double)dx) : q.z;
                const uint32_t nx = (uint32_t)(small2 + (double)((x - xmin) / dx));
                const uint32_t ny = (uint32_t)(small2 + (double)((y - ymin) / dx));
                const uint32_t nz = (uint32_t)(small2 + (double)((z - zmin) / dx));
                const uint32_t cellNo = ny * ncx + nz * (ncx * ncy) + nx;
                const long c = (long)cellNo;
                const long k = c / ((long)ncy * ncx);
                const long j = (c - k * (long)ncy * ncx) / ncx;
                q.i = (int)(c - (k * (long)ncy + j) * ncx);
                q.j = (int)j;
                q.k = (int)k;
            }
        } else {
            q.x = p[0]; q.z = p[1]; q.y = 0;
            const int fi = first_match(xmin, dx, ncx + 1, q.x);
            const int fk = first_match(zmin, dz, ncz + 1, q.z);
            if (fi >= 0 && fk >= 0) {
                q.on_node = 1; q.i = fi; q.k = fk;
            } else {
                // Grid2Drn::getCellNo uses `small` (ttcr/Grid2Drn.h:173-179)
                const double small = 1.e-4;
                const T x = (double)(xmax - q.x) < small ? (T)((double)xmax - .5 * (double)dx) : q.x;
                const T z = (double)(zmax - q.z) < small ? (T)((double)zmax - .5 * (double)dz) : q.z;
                const uint32_t nx = (uint32_t)(small + (double)((x - xmin) / dx));
                const uint32_t nz = (uint32_t)(small + (double)((z - zmin) / dz));
                const long c = (long)(uint32_t)(nx * ncz + nz);
                q.i = (int)(c / ncz);
                q.k = (int)(c - (long)q.i * ncz);
            }
        }
        return q;
    }

    // ---- sweeps -----------------------------------------------------------------------
    // What the kernel choice depends on (fsm_sweep_plan.h), for `entries` batch entries (slot groups / slots) swept together
    SweepFacts facts(int entries) const {
        SweepFacts f;
        fsm_sweep_tiles<T>(f, dim);
        f.weno = weno;
        f.rot45 = rotated && dx == dz;
        f.n_patches = n_patches; f.NF = geom.NF; f.NJ = geom.NJ; f.NK = geom.NK; f.nbf = nbf; f.cdirty_wpu = cdirty_wpu; f.n_launch = n_launch;
        f.slab_bits = 32 * FSM_SLAB_WORDS; f.cd_words = FSM_CD_WORDS;
        f.NS = NS;
        f.opt.mode = mode; f.opt.skip = skip; f.opt.lone_chunk = lone_chunk; f.opt.arith = arith;
        f.stage = stage; f.probe_skip = probe_skip; f.batch = entries;
        return f;
    }
    bool persistent_now() const { return fsm_persistent(facts(0)); }
    bool skip_now(int entries) const { return fsm_skip(facts(entries), tune); }

    // Sweep direction d: which axes run backwards, and the sheared copy of the slowness that direction reads.
    // 3-D: ttcr/Grid3Drn.h:2816-2899.  2-D direction order (i+,j+), (i-,j+), (i-,j-), (i+,j-)  (ttcr/Grid2Drn.h:717-751);
    // here F = z (the reference's j), J = x (the reference's i)
    void set_direction(SweepArgs<T>& a, int d) const {
        static const int RX2[4] = {0, 1, 1, 0}, RZ2[4] = {0, 0, 1, 1};
        int fam;
        if (dim == 3) {
            a.rf = d & 1; a.rj = (d >> 1) & 1; a.rk = (d >> 2) & 1;
            a.rev = a.rk;
            fam = (a.rf ^ a.rk) | ((a.rj ^ a.rk) << 1);
        } else {
            a.rj = RX2[d]; a.rf = RZ2[d]; a.rk = 0;
            a.rev = a.rj;
            fam = a.rf ^ a.rj;
        }
        a.s_sheared = d_ssh.p + (size_t)fam * ssh_stride;
    }

    // The sweeps of one iteration as the plan has them: one whole-iteration launch, one launch per sweep, or one per tile wavefront
    void launch_sweeps(const SweepPlan& p) {
        if (p.arith_needs_xs) throw ValueError("option 'arith' = 1 needs whole-iteration launches (option 'mode' = 2)");
        if (!sweep_kernel_exists<T>(p)) throw std::logic_error("no such sweep kernel (" + fsm_sweep_name(p) + ")");
        PersistArgs<T> pa;
        SweepArgs<T>& a = pa.s;
        a.tt = d_tt.p;
        a.ts = NS;
        a.lmask = d_lmask.p;
        a.frozen = d_mask.p;
        a.bbox = d_bbox.p;
        a.change = d_change.p;
        a.slots = d_slots.p;
        a.tiles = nullptr;
        a.g = geom;
        a.prof = d_prof.p;
        a.mask_words = (uint32_t)mask_words;
        a.dx = dx;
        a.dz = dz;
        a.w = 0;
        a.variant = dim == 3 ? 0 : (dx == dz ? 1 : 2);
        const int ndir = dim == 3 ? 8 : 4;
        if (p.persistent) {
            pa.sync = d_sync.p;
            pa.n_patches = n_patches;
            pa.batch = p.batch;
            pa.stamp = d_stamp.p;
            pa.iter_ptr = d_iter.p;
            pa.evals = d_evals.p;
            pa.nbf = nbf; pa.nbj = nbj; pa.nbk = nbk;
            pa.ndir = ndir;
            pa.skip = p.skip;
            pa.cmap = d_cmap.p;
            pa.cw = cmap_words;
            pa.cdirty = d_cdirty.p;
            pa.cdw = cdirty_wpu;
            pa.sw = p.sw ? d_sw.p : nullptr;
            pa.n_sw_groups = n_groups();
            pa.n_sw_sweeps = sw_sweeps;
            pa.fill_dst = nullptr;
            pa.fill_slice = 0;
            pa.fill_n = 0;
            if (p.XS) {
                pa.order = d_order_xs[p.H == 2 ? 1 : 0][p.tickets == SweepPlan::XS_BY_TIME ? 1 : 0].p;
                pa.ssh = d_ssh.p;
                pa.ssh_stride = ssh_stride;
                pa.dir = 0;
                a.rf = a.rj = a.rk = a.rev = 0;
                a.s_sheared = nullptr;
                pa.timeout_ticks = 1000000000ull;  // 10 s at 100 MHz: a unit may wait for most of the previous sweep
                if (fill_arm) {
                    // (solve_batch: first launch of a call that restarts every slot) the spare set, one slice per ticket of this launch
                    pa.fill_dst = d_tt_alt.p;
                    pa.fill_n = n_nodes * tt_fields();
                    pa.fill_slice = fsm_fill_slice_len(pa.fill_n, (size_t)n_patches * p.batch * ndir, 16 / sizeof(T));
                    fill_arm = false;
                    fill_in_flight = true;
                }
                launch_sweep_kernel<T>(p, pa, stream);
            } else {
                pa.order = d_order.p;
                pa.ssh = nullptr;
                pa.ssh_stride = 0;
                pa.timeout_ticks = 300000000ull;  // 3 s
                for (int d = 0; d < ndir; ++d) {
                    set_direction(a, d);
                    pa.dir = d;
                    // (no reset of tickets, progress words or change maps: launch epoch pa.iter_ptr[1] + d; the abort word is sticky
                    // within an iteration)
                    launch_sweep_kernel<T>(p, pa, stream);
                }
            }
            HIP_CHECK(hipGetLastError());
            return;
        }
        // one launch per tile wavefront
        for (int d = 0; d < ndir; ++d) {
            set_direction(a, d);
            for (int w = 0; w < n_launch; ++w) {
                if (tile_cnt[w] == 0) continue;
                a.w = w;
                a.tiles = d_tiles.p + tile_off[w];
                const dim3 grid(tile_cnt[w], 1, p.batch);
                if (dim == 3) fsm_sweep_tile<T, TileCfg<T, 3>::PJ, TileCfg<T, 3>::PK, TileCfg<T, 3>::BL, true><<<grid, dim3(p.block), 0, stream>>>(a);
                else fsm_sweep_tile<T, TileCfg<T, 2>::PJ, TileCfg<T, 2>::PK, TileCfg<T, 2>::BL, false><<<grid, dim3(p.block), 0, stream>>>(a);
            }
        }
        HIP_CHECK(hipGetLastError());
    }

    // Interleaved field layout: traveltime fields are stored in groups of NS sources,
    // T[group][node][NS] (NS = 2 when the grid has at least two slots).  The persistent kernel then
    // marches the NS sources of a group together: one address computation, one 8-byte load/store
    // and one LDS access serve both, and the per-level bookkeeping is shared.
    int NS = 1;
    bool ns_window = false;       // the grid may change its layout between calls (fsm_pair_layout)
    int pair_layout = -1;         // option "pair_layout": -1 (default) by the rule above, 0 one field per workgroup, 1 pairs (grids in the window only)
    double last_eval_frac = -1;   // evaluated / all node updates of the last batch that restarted every slot (-1: none yet)
    // Called at the top of a batch that restarts EVERY slot (no field of an earlier call survives it): pairs (NS = 2) or one field per
    // workgroup (NS = 1) for this and the following calls.  Nothing else depends on the layout across calls: stamps, change maps, sweep
    // tallies and snapshots are per solve, the second set of fields is filled with max() whatever its layout, host-side results are per slot.
    void choose_layout() {
        if (!ns_window) return;
        int want = NS;
        if (pair_layout >= 0) want = pair_layout ? 2 : 1;
        else if (last_eval_frac >= 0) want = NS == 2 ? (last_eval_frac < tune.layout_lo ? 1 : 2) : (last_eval_frac > tune.layout_hi ? 2 : 1);
        if (want == NS) return;
        NS = want;
        graph_plans[0].batch = graph_plans[1].batch = -1;   // (captured launches hold the layout)
        for (int q = 0; q < n_slots; ++q) phys[q] = q;
    }
    int n_groups() const { return (n_slots + NS - 1) / NS; }
    // fields of a set (d_tt, d_tt_alt): an odd slot count is padded to whole pairs only where the pair layout is or may come in use
    size_t tt_fields() const { return (size_t)n_slots + ((ns_window || NS == 2) ? (size_t)(n_slots & 1) : 0); }
    T* tt_ptr(int slot) const { return d_tt.p + (size_t)(slot / NS) * n_nodes * NS + slot % NS; }
    bool prefill_on() const {
        if (prefill >= 0) return prefill != 0;
        const size_t bytes = n_nodes * tt_fields() * sizeof(T);
        if (bytes < ((size_t)64 << 20)) return false;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
        return d_tt_alt.p || (2 * bytes <= total_b / 2 && bytes + ((size_t)1 << 30) <= free_b);
    }
    // The spare set filled by the units of the call's first sweep launch (fsm_sweep_unit: slice `ticket` at ticket draw) instead of by
    // fsm_fill on the side stream behind the call, which a caller that comes back at once waits for (512^3 x 64: 6-7 ms of a 180 ms
    // step).  Only for a call that restarts every slot, with a spare set to fill, whose first launch is a whole-iteration launch of
    // fsm_sweep_persistent issued directly (a captured launch would be replayed with the fill armed).  -1 (default): launches with at
    // least skip_units_min units per sweep of a 3-D grid -- those are bound by throughput; a lone source or a small batch lives on the
    // hop of its patch wavefront, and a burst of stores in front of a unit's first drain would sit on that path.
    bool fill_arm = false;         // the next whole-iteration launch carries the fill (taken by launch_sweeps)
    bool fill_in_flight = false;   // ... and it did
    bool inline_fill_now(int entries) const {
        if (prefill_inline == 0 || !d_tt_alt.p || d_tt_alt.n < n_nodes * tt_fields()) return false;
        if (mode != 2 || stage != 0 || use_graph >= 2) return false;
        if (prefill_inline == 1) return true;
        // (measured, 512^3 x 64, profiles/inline_prefill: 182.0 -> 179.1 ms per step with the reference's arithmetic; the tolerance-grade
        // kernels march faster and sit nearer the memory system's limit -- there the stores cost the launch more than the wait they
        // replace, 147.5 -> 148.5 ... 149.4 ms -- and keep the side stream)
        const SweepFacts f = facts(entries);
        return dim == 3 && !fsm_fast_arith(f) && fsm_units_per_sweep(f) >= tune.skip_units_min;
    }

    int stage = 0;  // 0: first-order sweeps, 1: WENO3 sweeps (persistent kernel only)
    bool probe_skip = true;      // what a launch in the probe window does now (SweepTuning::skip_probe_min)
    int probe_off_calls = 0;     // solves in the window since skipping was switched off
    int cdirty_wpu = 1;   // words of dirty bits per unit
    size_t cdirty_words() const { return (size_t)n_patches * n_slots * 8 * cdirty_wpu; }

    // Grid2Drn::sweep45 for every source of the batch (entries as handed to the sweep kernels)
    void launch_sweep45(int batch) {
        Sweep45Args<T> a;
        a.tt = d_tt.p;
        a.s = d_s.p;
        a.frozen = d_mask.p;
        a.change = d_change.p;
        a.slots = d_slots.p;
        a.lmask = d_lmask.p;
        a.ts = NS;
        a.by_group = persistent_now() ? 1 : 0;
        a.nnx = (int)ncx + 1;
        a.nnz = (int)ncz + 1;
        a.n_nodes = n_nodes;
        a.mask_words = (uint32_t)mask_words;
        a.dx = dx;
        const int blocks = a.by_group ? batch * NS : batch;
        // rows in sequence, a row in parallel: four row buffers of nnz+2 values in LDS (fits up to ~10 000 fp32 /
        // ~5 000 fp64 nodes along z); wider grids take the strip kernel with its level ring
        const size_t smem = 4 * ((size_t)a.nnz + 2) * sizeof(T);
        if (smem <= 156 * 1024 && !sweep45_strips) {
            const int threads = (int)std::min<size_t>(1024, (((size_t)a.nnz + 63) / 64) * 64);
            fsm_sweep45_rows<T><<<blocks, threads, smem, stream>>>(a);
        } else {
            constexpr int NTMAX = sizeof(T) == 4 ? 1024 : 512;
            if (a.nnx + 2 <= 256) fsm_sweep45<T, 256><<<blocks, 256, 0, stream>>>(a);
            else fsm_sweep45<T, NTMAX><<<blocks, NTMAX, 0, stream>>>(a);
        }
        HIP_CHECK(hipGetLastError());
    }

    void issue_sweeps(const SweepPlan& p) {
        launch_sweeps(p);
        if (dim == 2 && rotated && !weno && dx == dz) launch_sweep45(p.batch);
    }

    void run_iteration(int batch) {
        const SweepPlan plan = fsm_sweep_plan(facts(batch), tune);
        last_kernel = fsm_sweep_name(plan);
        if (use_graph >= 2 || (use_graph == 1 && !plan.persistent)) {
            hipGraph_t& graph = graphs[stage];
            hipGraphExec_t& graph_exec = graph_execs[stage];
            if (!graph_exec || plan != graph_plans[stage]) {
                if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
                if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
                HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                try {
                    issue_sweeps(plan);
                } catch (...) {
                    hipGraph_t junk = nullptr;
                    (void)hipStreamEndCapture(stream, &junk);
                    if (junk) (void)hipGraphDestroy(junk);
                    throw;
                }
                HIP_CHECK(hipStreamEndCapture(stream, &graph));
                HIP_CHECK(hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
                graph_plans[stage] = plan;
            }
            HIP_CHECK(hipGraphLaunch(graph_exec, stream));
        } else {
            issue_sweeps(plan);
        }
        timing.launches += plan.launches;
    }

    // One batch: sources src_ids[b] solved concurrently, source b in slot slot_ids[b].
    // ---- the reference's stopping rule where it matters (option stopping_rule = 1) ---------------------------------
    // Grid3Drnfs::raytrace (ttcr/Grid3Drnfs.h:141-152) sums abs(times[n] - T[n]) over the nodes in order, in T1.  The sweep kernels
    // accumulate the same quantity as an fp64 sum of decreases; the two agree to a few percent near eps * N at 1.3e8 fp32 nodes
    // (profiles/r03/stopping_rule_512.txt), so an iteration whose fp64 change lies within [1/2, 16] x eps * N (fp64 grids: 1e-6
    // either side) is decided by the reference's own sum, computed by fsm_reference_change from a snapshot of the field.  The
    // snapshot of a slot group is taken before an iteration when the change of the iteration before was below 1e4 x 16 x eps * N
    // (consecutive iterations differ by factors of 4 - 40); an iteration that lands in the window without one is decided by the
    // fp64 sum and counted (reference_sums_missed).
    std::map<int, DevBuf<T>> snap;            // slot group -> field(s) before the current iteration
    std::vector<int> snap_iter;               // [group] iteration (stage-local, 1-based) the snapshot belongs to, 0: none
    std::vector<double> prev_change;          // [slot] fp64 change of the iteration before (inf: none yet)
    std::vector<double> prev2_change;         // [slot] ... and of the one before that
    bool snap_always = false;                 // this solve missed a snapshot once: no more predictions
    std::vector<int> snap_T;                  // [group] global iteration index the snapshot is the field in front of (-1: none / not to be trusted)
    bool stamps_ok = false;                   // every iteration of this solve (and stage) so far ran a kernel that keeps the dirty-brick stamps
    int iter_T = 0;                           // global index of the iteration that runs / has just run (sweep numbers of the stamps: ndir * iter_T + 1 ...)
    bool stamps_live_for(int entries) const { return (stopping_shortcuts & 1) && dim == 3 && !weno && persistent_now() && skip_now(entries) && n_nodes * (size_t)NS < ((size_t)1 << 31); }
    // the pass over the fields of group gi and its snapshot (fsm_refsum_terms): terms of the sources asked for (x0 / x1, counts c0 / c1;
    // all nullptr: the snapshot alone); since_T >= 0: only the bricks that changed in iteration since_T or later
    void terms_pass(int gi, T* x0, T* x1, unsigned* c0, unsigned* c1, int since_T) {
        RefTermsArgs<T> ta;
        ta.cur = d_tt.p + (size_t)gi * n_nodes * NS;
        ta.old = snap[gi].p;
        ta.x[0] = x0; ta.x[1] = x1;
        ta.cnt[0] = c0; ta.cnt[1] = c1;
        ta.n_nodes = (uint32_t)n_nodes;
        ta.ns = NS;
        constexpr int V = 16 / (int)sizeof(T);
        const size_t n_el = n_nodes * (size_t)NS;
        const bool vec = n_el % V == 0 && ((uintptr_t)ta.cur | (uintptr_t)ta.old) % 16 == 0;
        const int nodes_per_vec = vec ? std::max(1, V / NS) : 1;
        const bool bricks = since_T >= 0 && geom.NF % nodes_per_vec == 0;
        ta.stamp = bricks ? d_stamp.p + (size_t)gi * n_bricks : nullptr;
        ta.thr = (dim == 3 ? 8 : 4) * since_T + 1;
        ta.NF = geom.NF; ta.NJ = geom.NJ; ta.nbf = nbf; ta.nbj = nbj;
        const unsigned nblk = (unsigned)((n_nodes + FSM_REFSUM_CB - 1) / FSM_REFSUM_CB);
        const unsigned blocks = std::min(nblk, 8192u);
        if (vec) fsm_refsum_terms<T, V><<<blocks, 256, 0, stream>>>(ta);
        else fsm_refsum_terms<T, 1><<<blocks, 256, 0, stream>>>(ta);
        HIP_CHECK(hipGetLastError());
    }
    DevBuf<size_t> d_ref_off;
    DevBuf<T> d_ref_out;
    double window_lo() const { return sizeof(T) == 4 ? 0.5 : 1.0 - 1e-6; }
    double window_hi() const { return sizeof(T) == 4 ? 16.0 : 1.0 + 1e-6; }
    void snapshots_before_iteration(const std::vector<int>& active, int it_next) {
        if (!stopping_rule || fixed_iters > 0) return;
        if ((int)snap_iter.size() != n_groups()) snap_iter.assign(n_groups(), 0);
        // a snapshot costs a copy of the field(s) of a slot group: taken whenever the iteration may land in the window -- the change
        // of the iteration before, continued with the decrease it showed against the one before it (consecutive iterations differ
        // by factors of 4 - 40, a factor changes by less than 8 from one iteration to the next) comes within the window; with one
        // iteration to go by, within 1e3 windows --, before the first iteration of the WENO stage (its `times` is the last
        // first-order field: the change can be anything), and always while the copy is cheap (up to 2^24 nodes)
        const bool cheap = n_nodes * (size_t)NS <= ((size_t)1 << 24);
        std::vector<char> done(n_groups(), 0);
        for (int s2 : active) {
            const int gi = s2 / NS;
            if (done[gi]) continue;
            bool may = prev_change[s2] < 1e3 * window_hi() * (double)epsilon;
            if (may && (int)prev2_change.size() == n_slots && std::isfinite(prev2_change[s2]) && prev2_change[s2] > 0) {
                const double r = std::min(1.0, prev_change[s2] / prev2_change[s2]);
                may = prev_change[s2] * r / 8.0 <= window_hi() * (double)epsilon;
            }
            // (a miss -- an iteration that landed in the window without a snapshot, decided by the fp64 sum -- shows the prediction does
            // not hold for this model: from then on every iteration of the solve is snapshotted)
            if (!(cheap || (stage == 1 && it_next == 1) || may || snap_always)) continue;
            if (it_next == 1 && stage == 0) continue;   // (the first iteration of a solve: its change is infinite -- every node comes down from max())
            done[gi] = 1;
            if (snap_iter[gi] == it_next) continue;     // (brought up to date by the pass that wrote the terms of the last sum: decide_go_on)
            DevBuf<T>& b = snap[gi];
            b.reserve(n_nodes * (size_t)NS);
            if ((int)snap_T.size() != n_groups()) snap_T.assign(n_groups(), -1);
            // (a snapshot that was right in front of an earlier iteration: the bricks that changed since then, by their stamps)
            if (stamps_ok && snap_T[gi] >= 0 && n_nodes * (size_t)NS < ((size_t)1 << 32)) terms_pass(gi, nullptr, nullptr, nullptr, nullptr, snap_T[gi]);
            else HIP_CHECK(hipMemcpyAsync(b.p, d_tt.p + (size_t)gi * n_nodes * NS, n_nodes * (size_t)NS * sizeof(T), hipMemcpyDeviceToDevice, stream));
            snap_iter[gi] = it_next;
            snap_T[gi] = iter_T;
        }
    }
    // The reference's `change` of one field: sum over the nodes, in order, in T1, of abs(times[n] - T[n]).  stopping_rule = 2: the
    // one-chain kernel (fsm_reference_change: 1.3e8 dependent additions for a 512^3 field); otherwise the same sum computed in
    // parallel, exactly (fsm_refsum_*, fsm_kernels.h): rounds of a tile scan over a window of the field + one workgroup that finds
    // where the running sum leaves its binade; the window follows the distance between such places.
    DevBuf<RefSumState> d_rs_state;
    DevBuf<RefSum4<T>> d_rs_tiles;
    DevBuf<T> d_rc_a, d_rc_b;
    size_t rs_fields_max = 16;               // fields of one batch of decide_go_on (0: no room for the compact arrays on this device)
    DevBuf<T> d_rs_x, d_rs_xc;               // [asked field][n_nodes, padded] terms of the sums of one decision; the non-zero ones, in order
    DevBuf<unsigned> d_rs_cnt;               // [asked field][block of FSM_REFSUM_CB nodes] non-zero terms
    DevBuf<unsigned long long> d_rs_off, d_rs_n, d_rs_n2;   // ... exclusive scan of them; [asked field] number of terms
    void reference_change_host(const void* times, const void* field, bool parallel, void* out) override {
        HIP_CHECK(hipSetDevice(device));
        d_rc_a.reserve(n_nodes);
        d_rc_b.reserve(n_nodes);
        HIP_CHECK(hipMemcpyAsync(d_rc_a.p, field, n_nodes * sizeof(T), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rc_b.p, times, n_nodes * sizeof(T), hipMemcpyHostToDevice, stream));
        *(T*)out = reference_change(d_rc_a.p, d_rc_b.p, 1, !parallel);
    }
    T reference_change(const T* cur, const T* old, int stride, bool one_chain) {
        std::vector<const T*> c{cur}, o{old};
        return reference_changes(c, o, stride, one_chain, std::numeric_limits<T>::infinity())[0];
    }
    DevBuf<const T*> d_rs_ptrs;
    DevBuf<unsigned> d_rs_arrived;
    // several fields at once: the rounds of all of them run side by side, enqueued in bunches (the state of every field stays on the
    // device between its rounds: start, sum, window; a field that is done lets its later rounds pass)
    // stop_at: a field is done once its running sum has reached this value (the sum only grows; the value returned is then a lower bound)
    // d_n: [field] number of terms on the device (compacted fields: fsm_refsum_scan's totals); nullptr: n_nodes each
    std::vector<T> reference_changes(const std::vector<const T*>& cur, const std::vector<const T*>& old, int stride, bool one_chain, T stop_at,
                                     const unsigned long long* d_n = nullptr, const std::vector<unsigned long long>* h_n_known = nullptr) {
        const size_t nf = cur.size();
        std::vector<T> out(nf, (T)0);
        if (one_chain) {
            d_ref_off.reserve(1);
            d_ref_out.reserve(1);
            for (size_t f = 0; f < nf; ++f) {
                RefChangeArgs<T> ra;
                ra.cur = cur[f];
                ra.old = old[f];
                const size_t zero = 0;
                HIP_CHECK(hipMemcpyAsync(d_ref_off.p, &zero, sizeof(size_t), hipMemcpyHostToDevice, stream));
                ra.off = d_ref_off.p;
                ra.out = d_ref_out.p;
                ra.n_nodes = n_nodes;
                ra.stride = stride;
                fsm_reference_change<T><<<1, 256, 0, stream>>>(ra);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(&out[f], d_ref_out.p, sizeof(T), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
            return out;
        }
        const size_t tiles_per_field = FSM_REFSUM_WMAX / FSM_REFSUM_TILE;
        d_rs_state.reserve(2 * nf);
        d_rs_tiles.reserve(nf * tiles_per_field);
        d_rs_ptrs.reserve(2 * nf);
        d_rs_arrived.reserve(nf);
        HIP_CHECK(hipMemsetAsync(d_rs_arrived.p, 0, nf * sizeof(unsigned), stream));
        std::vector<RefSumState> st(nf, RefSumState{0ull, 0ull, FSM_REFSUM_WMIN, 0ull});
        std::vector<const T*> ptrs(cur);
        ptrs.insert(ptrs.end(), old.begin(), old.end());
        HIP_CHECK(hipMemcpyAsync(d_rs_state.p, st.data(), nf * sizeof(RefSumState), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rs_ptrs.p, ptrs.data(), 2 * nf * sizeof(const T*), hipMemcpyHostToDevice, stream));
        RefSumArgs<T> ra;
        ra.cur = d_rs_ptrs.p;
        ra.old = d_rs_ptrs.p + nf;
        std::vector<unsigned long long> h_n(nf, (unsigned long long)n_nodes);
        unsigned long long n_max = n_nodes;
        if (!d_n) {
            d_rs_n.reserve(nf);
            HIP_CHECK(hipMemcpyAsync(d_rs_n.p, h_n.data(), nf * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            d_n = d_rs_n.p;
        } else {
            // compacted fields: their lengths size the launches (windows that always reach to the end of the field were tried: fewer
            // rounds, 176 against 240 per solve of bench.py's heterogeneous leg, but 136 us each against 29 -- the scan is arithmetic)
            if (h_n_known) h_n = *h_n_known;
            else {
                HIP_CHECK(hipMemcpyAsync(h_n.data(), d_n, nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
            n_max = 0;
            for (size_t f = 0; f < nf; ++f) n_max = std::max(n_max, h_n[f]);
            if (n_max == 0) return out;   // (no node changed at all: the sum of no terms)
        }
        ra.n = d_n;
        ra.stride = stride;
        ra.st = d_rs_state.p;
        ra.tiles = d_rs_tiles.p;
        ra.arrived = d_rs_arrived.p;
        ra.stop_at = stop_at;
        const unsigned max_tiles = (unsigned)std::min<unsigned long long>(tiles_per_field, (n_max + FSM_REFSUM_TILE - 1) / FSM_REFSUM_TILE);
        ra.round = 0;   // (round r reads buffer r & 1 of the states and writes the other one; the initial states sit in buffer 0)
        fsm_refsum_head<T><<<(unsigned)nf, 256, 0, stream>>>(ra);   // (... written by the pass over the head of every field)
        static const bool trace = std::getenv("TTCR_FSM_REFSUM_TRACE") != nullptr;   // tuning: one round per bunch, its state and wall clock on stderr
        for (int bunch = trace ? 1 : 16;; bunch = trace ? 1 : 8) {   // (rounds are enqueued in bunches: a field that is done lets the rest of its bunch pass)
            const auto t_b = std::chrono::steady_clock::now();
            for (int r = 0; r < bunch; ++r, ++ra.round) fsm_refsum_round<T><<<dim3(std::min(max_tiles, 1024u), (unsigned)nf), 256, 0, stream>>>(ra);
            HIP_CHECK(hipGetLastError());
            refsum_rounds += bunch;
            HIP_CHECK(hipMemcpyAsync(st.data(), d_rs_state.p + (size_t)(ra.round & 1) * nf, nf * sizeof(RefSumState), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            if (trace) {
                std::fprintf(stderr, "[refsum] round %3d  %7.1f us ", ra.round, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_b).count());
                for (size_t f = 0; f < nf; ++f) std::fprintf(stderr, " | start %llu of %llu window %llu", st[f].start, h_n[f], st[f].window);
                std::fprintf(stderr, "\n");
            }
            bool done = true;
            for (size_t f = 0; f < nf; ++f) done = done && st[f].start >= h_n[f];
            if (done) break;
        }
        for (size_t f = 0; f < nf; ++f) {
            if constexpr (sizeof(T) == 4) { const unsigned b = (unsigned)st[f].bits; std::memcpy(&out[f], &b, 4); } else { std::memcpy(&out[f], &st[f].bits, 8); }
        }
        return out;
    }
    // go on after this iteration?  (active slot s2, its fp64 change c, iteration `it` just done)
    std::vector<char> decide_go_on(const std::vector<int>& active, int it) {
        std::vector<char> go(active.size(), 0);
        std::vector<int> ask;
        if ((int)ref_change_last.size() != n_slots) ref_change_last.assign(n_slots, std::nan(""));
        for (int s2 : active) ref_change_last[s2] = std::nan("");
        for (size_t q = 0; q < active.size(); ++q) {
            const int s2 = active[q];
            const double c = h_change[s2];
            go[q] = c >= (double)epsilon;
            if (!stopping_rule || !(c >= window_lo() * (double)epsilon && c <= window_hi() * (double)epsilon)) continue;
            if ((int)snap_iter.size() == n_groups() && snap_iter[s2 / NS] == it) ask.push_back((int)q);
            else { ++reference_sums_missed; snap_always = true; }
        }
        if (ask.empty()) return go;
        std::vector<T> res(ask.size());
        std::vector<char> res_known(ask.size(), 0), res_go(ask.size(), 0);   // the sum itself / the side of eps * N it provably lies on
        if (stopping_rule == 2 || n_nodes * (size_t)NS >= ((size_t)1 << 32)) {
            std::vector<const T*> curs(ask.size()), olds(ask.size());
            for (size_t a = 0; a < ask.size(); ++a) {
                const int s2 = active[ask[a]], gi = s2 / NS;
                curs[a] = d_tt.p + (size_t)gi * n_nodes * NS + s2 % NS;
                olds[a] = snap[gi].p + s2 % NS;
            }
            res = reference_changes(curs, olds, NS, stopping_rule == 2, epsilon);   // (asked: change >= epsilon)
            res_known.assign(ask.size(), 1);
        } else {
            // The terms of the fields that were asked for, compact (fsm_refsum_terms: one pass over a group's fields and its snapshot, which
            // leaves the snapshot equal to the current field -- the one the next iteration would take), then the non-zero ones alone in
            // node order (fsm_refsum_scan / _compact), then the ordered pass over those.  Up to 16 fields at a time (whole groups).
            const size_t pitch = (n_nodes + FSM_REFSUM_CB - 1) / FSM_REFSUM_CB * FSM_REFSUM_CB;
            const unsigned nblk = (unsigned)(pitch / FSM_REFSUM_CB);
            for (size_t a0 = 0; a0 < ask.size();) {
                // (two arrays of n_nodes values per field of a batch: where the device has no room for 16 fields the batches get smaller,
                // and a grid that has none for a pair goes by the strided fields and whole-field snapshots, as in round 5)
                size_t a1 = a0, nf = 0;
                bool room = false;
                while (rs_fields_max >= 2) {
                    a1 = a0;
                    while (a1 < ask.size() && (a1 - a0 + 1 < rs_fields_max || (a1 > a0 && active[ask[a1]] / NS == active[ask[a1 - 1]] / NS))) ++a1;
                    nf = a1 - a0;
                    try {
                        d_rs_x.reserve(nf * pitch);
                        d_rs_xc.reserve(nf * pitch);
                        d_rs_cnt.reserve(nf * (size_t)nblk);
                        d_rs_off.reserve(nf * (size_t)nblk);
                        d_rs_n.reserve(std::max<size_t>(nf, 64));
                        room = true;
                        break;
                    } catch (const DeviceError&) {
                        (void)hipGetLastError();
                        d_rs_x.release();
                        d_rs_xc.release();
                        rs_fields_max = rs_fields_max > 2 ? std::max<size_t>(2, rs_fields_max / 2) : 0;
                    }
                }
                if (!room) {
                    std::vector<const T*> curs(ask.size() - a0), olds(ask.size() - a0);
                    for (size_t a = a0; a < ask.size(); ++a) {
                        const int s2 = active[ask[a]], gi = s2 / NS;
                        curs[a - a0] = d_tt.p + (size_t)gi * n_nodes * NS + s2 % NS;
                        olds[a - a0] = snap[gi].p + s2 % NS;
                    }
                    const std::vector<T> r = reference_changes(curs, olds, NS, false, epsilon);
                    for (size_t a = a0; a < ask.size(); ++a) { res[a] = r[a - a0]; res_known[a] = 1; }
                    break;
                }
                std::vector<const T*> curs(nf), olds(nf, nullptr);
                for (size_t a = a0; a < a1; ++a) {
                    curs[a - a0] = d_rs_xc.p + (a - a0) * pitch;
                    const int gi = active[ask[a]] / NS;
                    if (a > a0 && active[ask[a - 1]] / NS == gi) continue;   // (with the source in front of it: `active` is in slot order)
                    T* xp[2] = {nullptr, nullptr};
                    unsigned* cp[2] = {nullptr, nullptr};
                    for (size_t b = a; b < a1 && active[ask[b]] / NS == gi; ++b) {
                        xp[active[ask[b]] % NS] = d_rs_x.p + (b - a0) * pitch;
                        cp[active[ask[b]] % NS] = d_rs_cnt.p + (b - a0) * (size_t)nblk;
                    }
                    // (the snapshot is the field in front of this iteration: the bricks this iteration changed hold all the terms)
                    const bool bricks = stamps_ok && (int)snap_T.size() == n_groups() && snap_T[gi] == iter_T;
                    terms_pass(gi, xp[0], xp[1], cp[0], cp[1], bricks ? iter_T : -1);
                    snap_iter[gi] = it + 1;
                    if ((int)snap_T.size() != n_groups()) snap_T.assign(n_groups(), -1);
                    snap_T[gi] = iter_T + 1;
                }
                const dim3 cgrid(std::min(nblk, 4096u), (unsigned)nf);
                fsm_refsum_scan<0><<<(unsigned)nf, 1024, 0, stream>>>(d_rs_cnt.p, d_rs_off.p, nblk, d_rs_n.p);
                HIP_CHECK(hipGetLastError());
                // With M non-zero terms the sequential T1 sum lies within gamma = M u / (1 - M u) of the exact one (recursive summation of
                // non-negative terms, u the unit roundoff of T1; zeros are added exactly), and the fp64 sum of decreases the sweep kernels
                // hand over is the exact one to within m: every thread adds the decreases of its nodes of a unit -- at most
                // NF + NJ + NK of them -- in T1 before they go to the fp64 atomics.  Where these bounds put the reference's sum on one
                // side of eps * N, `change >= epsilon` is decided as the reference decides it without computing the sum (option
                // "stopping_shortcuts", bit 1); the ordered pass runs for the rest.
                // What m has to cover, kernel by kernel that adds to d_change -- the T1 additions a thread makes before it converts
                // its sum to double (each term c - t is one more rounding in T1; the wave reduction and the atomics are fp64):
                //   fsm_sweep_unit (every persistent kernel)   NF per unit and source: a thread keeps one column (jp, kp) of the patch and
                //                                              meets one node of it per level, ip = L - jp - kp in [0, NF), whatever the
                //                                              chunk length (8, 16: the chunks only cut the column up) and NS (dec[l] is per
                //                                              source); the sum starts from zero in every unit, looped workgroups included
                //   fsm_sweep_tile (mode 0)                    BL per tile: 16 levels in 3-D, 32 in 2-D
                //   fsm_sweep45, fsm_sweep45_rows              none: the terms are added in double (in T1 they were 4 ceil(nnx / S) nnz and
                //                                              4 nnx ceil(nnz / blockDim) -- 8192 x 64 fp32: 32 768 against NF+NJ+NK+64 = 8320)
                // n such additions of non-negative terms and the rounding of the terms are off by at most n u / (1 - n u) in all, and
                // n <= NF < NF + NJ + NK + 64 everywhere: m holds with a factor of two to spare (tests/test_change_sum_gpu.py measures it).
                std::vector<unsigned long long> h_m(nf);
                HIP_CHECK(hipMemcpyAsync(h_m.data(), d_rs_n.p, nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
                std::vector<size_t> need;
                for (size_t f = 0; f < nf; ++f) {
                    const double u = 0.5 * (double)std::numeric_limits<T>::epsilon(), mu = (double)h_m[f] * u;
                    const double c = h_change[active[ask[a0 + f]]], e = (double)epsilon;
                    if (host_prof) std::fprintf(stderr, "[host]   ask: slot %d iteration %d  fp64 change / (eps N) %.4f  non-zero terms %llu (M u = %.4f)\n", active[ask[a0 + f]], it, c / e, h_m[f], mu);
                    if (h_m[f] == 0ull) { res[a0 + f] = (T)0; res_known[a0 + f] = 1; continue; }   // (the sum of no terms)
                    if ((stopping_shortcuts & 2) && stage == 0 && mu < 0.25) {   // (first-order sweeps: a node only ever comes down)
                        const double g = mu / (1.0 - mu), m = 2.0 * (double)(geom.NF + geom.NJ + geom.NK + 64) * u + 1e-6;
                        if (c * (1.0 - m) * (1.0 - g) >= e) { res_go[a0 + f] = 1; continue; }
                        if (c * (1.0 + m) * (1.0 + g) < e) { res_go[a0 + f] = 0; continue; }
                    }
                    need.push_back(f);
                }
                if (!need.empty()) {
                    fsm_refsum_compact<T><<<cgrid, 256, 0, stream>>>(d_rs_x.p, d_rs_xc.p, pitch, n_nodes, d_rs_cnt.p, d_rs_off.p, nblk);
                    HIP_CHECK(hipGetLastError());
                    std::vector<const T*> c2(need.size()), o2(need.size(), nullptr);
                    std::vector<unsigned long long> m2(need.size());
                    for (size_t q = 0; q < need.size(); ++q) { c2[q] = curs[need[q]]; m2[q] = h_m[need[q]]; }
                    d_rs_n2.reserve(std::max<size_t>(need.size(), 64));
                    HIP_CHECK(hipMemcpyAsync(d_rs_n2.p, m2.data(), need.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
                    const std::vector<T> r = reference_changes(c2, o2, 1, false, epsilon, d_rs_n2.p, &m2);   // (asked: change >= epsilon)
                    for (size_t q = 0; q < need.size(); ++q) { res[a0 + need[q]] = r[q]; res_known[a0 + need[q]] = 1; }
                }
                a0 = a1;
            }
        }
        for (size_t a = 0; a < ask.size(); ++a) {
            go[ask[a]] = res_known[a] ? res[a] >= epsilon : res_go[a] != 0;   // `change >= epsilon`, both T1 (ttcr/Grid3Drnfs.h:153)
            if (res_known[a]) ref_change_last[active[ask[a]]] = (double)res[a];
            ++reference_sums;
        }
        return go;
    }
    std::vector<double> ref_change_last;   // [slot] the reference's sum of the iteration just decided, if it was decided with it (NaN: not)

    // TTCR_FSM_HOST_PROF=1: wall clock of the host-side phases of a call (stderr), tuning only
    bool host_prof = std::getenv("TTCR_FSM_HOST_PROF") != nullptr;
    std::chrono::steady_clock::time_point hp_t = std::chrono::steady_clock::now();
    void hp_mark(const char* what) {
        if (!host_prof) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - hp_t).count());
        hp_t = now;
    }
    void solve_batch(const std::vector<int>& slot_ids, const std::vector<int>& src_ids, const int* tx_off,
                     const T* tx, const T* t0) {
        const int nb = (int)slot_ids.size();
        hp_mark("(before solve_batch)");
        const int nc = ncoord();
        const long long node_updates_before = timing.node_updates;
        // reinit + initFSM (ttcr/Grid3Drnfs.h:92-100)
        size_t tot_pts = 0;
        for (int b = 0; b < nb; ++b) tot_pts += tx_off[src_ids[b] + 1] - tx_off[src_ids[b]];
        std::vector<InitPoint<T>> pts;
        pts.reserve(tot_pts);
        std::vector<size_t> first(nb);
        for (int b = 0; b < nb; ++b) {
            first[b] = pts.size();
            for (int n = tx_off[src_ids[b]]; n < tx_off[src_ids[b] + 1]; ++n) pts.push_back(locate(tx + (size_t)nc * n, t0[n]));
        }
        d_pts.reserve(std::max<size_t>(tot_pts, 1));
        HIP_CHECK(hipMemcpyAsync(d_pts.p, pts.data(), pts.size() * sizeof(InitPoint<T>), hipMemcpyHostToDevice, stream));
        for (int b = 0; b < nb; ++b)  // dirty-brick stamps: one set per slot group, "never changed"
            HIP_CHECK(hipMemsetAsync(d_stamp.p + (size_t)(slot_ids[b] / NS) * n_bricks, 0xFF, n_bricks * sizeof(int), stream));
        // reinit (Node3Dn::reinit): T = max() everywhere.  When every source of an interleaved group is
        // (re)started in this batch the group is one contiguous fill (full-line stores) instead of NS
        // strided passes.
        std::vector<char> group_filled(n_groups(), 0);
        // every slot of the grid restarted by this batch: take the fields the side stream has initialised since the last such call
        const bool all_slots = nb == n_slots && prefill_on();
        fill_arm = fill_in_flight = false;
        bool inline_filled = false;   // the spare set was filled by this call's first sweep launch, and that launch ended normally
        if (all_slots && alt_filled) {
            HIP_CHECK(hipStreamWaitEvent(stream, ev_fill, 0));
            std::swap(d_tt.p, d_tt_alt.p);
            std::swap(d_tt.n, d_tt_alt.n);
            std::swap(d_tt.guard, d_tt_alt.guard);
            alt_filled = false;
            ++prefill_swaps;
            graph_plans[0].batch = graph_plans[1].batch = -1;   // (captured launches hold the field pointer)
            std::fill(group_filled.begin(), group_filled.end(), 1);
        }
        if (NS > 1) {
            std::vector<int> cnt(n_groups(), 0);
            for (int b = 0; b < nb; ++b) cnt[slot_ids[b] / NS] += 1;
            for (int gi = 0; gi < n_groups(); ++gi) {
                if (cnt[gi] != NS || group_filled[gi]) continue;   // (group_filled: the fields came initialised from the side stream)
                const size_t n_el = n_nodes * (size_t)NS;
                const int blocks = (int)std::min<size_t>((n_el + 255) / 256, 16384);
                fsm_fill<T><<<blocks, 256, 0, stream>>>(d_tt.p + (size_t)gi * n_el, n_el, real_traits<T>::max(), 1);
                group_filled[gi] = 1;
            }
        }
        for (int b = 0; b < nb; ++b) {
            const int slot = slot_ids[b];
            T* tt = tt_ptr(slot);
            const int blocks = (int)std::min<size_t>((n_nodes + 255) / 256, 8192);
            if (!group_filled[slot / NS]) fsm_fill<T><<<blocks, 256, 0, stream>>>(tt, n_nodes, real_traits<T>::max(), NS);
            HIP_CHECK(hipMemsetAsync(d_mask.p + (size_t)slot * mask_words, 0, mask_words * sizeof(uint32_t), stream));
            InitArgs<T> ia;
            ia.tt = tt;
            ia.ts = NS;
            ia.slowness = d_s.p;
            ia.frozen = d_mask.p + (size_t)slot * mask_words;
            ia.bbox = d_bbox.p + 6 * (size_t)slot;
            ia.pts = d_pts.p + first[b];
            ia.n_pts = tx_off[src_ids[b] + 1] - tx_off[src_ids[b]];
            ia.npts = weno ? 2 : 1;  // frozen box of the WENO solver (ttcr/Grid3Drnfs.h:98-100)
            ia.nnx = ncx + 1;
            ia.nny = dim == 3 ? ncy + 1 : 1;
            ia.nnz = ncz + 1;
            ia.dx = dx; ia.dz = dz; ia.xmin = xmin; ia.ymin = ymin; ia.zmin = zmin;
            ia.dim = dim;
            ia.stamp = d_stamp.p + (size_t)(slot / NS) * n_bricks;
            ia.nbf = nbf; ia.nbj = nbj; ia.nbk = nbk;
            fsm_init_source<T><<<1, 128, 0, stream>>>(ia);
            niter[slot] = 0;
            niterw[slot] = 0;
            if (change_hist.empty()) { change_hist.resize(n_slots); change_histw.resize(n_slots); }
            if (ref_hist.empty()) { ref_hist.resize(n_slots); ref_histw.resize(n_slots); }
            change_hist[slot].clear();
            change_histw[slot].clear();
            ref_hist[slot].clear();
            ref_histw[slot].clear();
        }
        HIP_CHECK(hipGetLastError());
        hp_mark("reinit + initFSM issued");
        HIP_CHECK(hipStreamSynchronize(stream));  // pts vector goes out of scope below; also surfaces errors early
        hp_mark("reinit + initFSM done");

        // driver loop of Grid3Drnfs::raytrace, per source: first-order sweeps until the L1 change
        // drops below eps*N (ttcr/Grid3Drnfs.h:137-153); with weno3 a second loop of WENO sweeps with
        // the change reset (:104-136).  A source that converges leaves the batch (slot -1).
        const int maxit = fixed_iters > 0 ? fixed_iters : nitermax;
        const int ndir = dim == 3 ? 8 : 4;
        if (!sync_clean || launch_epoch > 0xfffff000u) {   // a solve that did not end normally (or 2^32 launches): start over
            HIP_CHECK(hipMemsetAsync(d_sync.p, 0, sync_words * sizeof(int), stream));
            HIP_CHECK(hipMemsetAsync(d_cmap.p, 0, (size_t)n_patches * n_slots * ndir * 2 * cmap_words * sizeof(unsigned long long), stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            launch_epoch = 1;
        }
        sync_clean = false;
        snap_always = false;
        // progress words: wiped once per solve (an ordinary stream operation, like the fills above); between the launches of
        // the solve the 2-bit epoch field tells this launch's values from the previous launch's
        if (persistent_now() || weno) HIP_CHECK(hipMemsetAsync(d_sync.p + 8, 0, (sync_words - 8) * sizeof(int), stream));
        if (persistent_now() || weno) HIP_CHECK(hipMemsetAsync(d_sync.p + 4, 0, sizeof(int), stream));
        HIP_CHECK(hipMemsetAsync(d_evals.p, 0, sizeof(unsigned long long) * n_slots, stream));
        HIP_CHECK(hipMemsetAsync(d_sw.p, 0, sizeof(unsigned long long) * (size_t)sw_sweeps * n_groups(), stream));
        if (d_cdirty.p) HIP_CHECK(hipMemsetAsync(d_cdirty.p, 0, cdirty_words() * sizeof(unsigned), stream));   // (no sweep before the first one)
        HIP_CHECK(hipEventRecord(ev0, stream));
        int it_total = 0;  // global iteration index: sweep numbers for the dirty-brick stamps
        for (stage = 0; stage < (weno ? 2 : 1); ++stage) {
            std::vector<int> active(slot_ids);
            int it = 0;
            prev_change.assign(n_slots, std::numeric_limits<double>::infinity());   // (the first iteration of a stage always runs: no snapshot)
            prev2_change.assign(n_slots, std::numeric_limits<double>::infinity());
            snap_iter.assign(n_groups(), 0);
            snap_T.assign(n_groups(), -1);
            stamps_ok = false;
            if ((int)ref_change_last.size() != n_slots) ref_change_last.assign(n_slots, std::nan(""));
            // batch entries: slot groups for the persistent kernel (with a lane mask), slots otherwise
            std::vector<int> groups;
            for (int s2 : slot_ids)
                if (groups.empty() || groups.back() != s2 / NS) groups.push_back(s2 / NS);
            while (!active.empty() && it < maxit) {
                int n_entries;
                if (persistent_now()) {
                    n_entries = (int)groups.size();
                    for (int b = 0; b < n_entries; ++b) {
                        int m2 = 0;
                        for (int s2 : active)
                            if (s2 / NS == groups[b]) m2 |= 1 << (s2 % NS);
                        h_slots[b] = m2 ? groups[b] : -1;
                        h_lmask[b] = m2;
                    }
                } else {
                    n_entries = nb;
                    for (int b = 0; b < nb; ++b) { h_slots[b] = b < (int)active.size() ? active[b] : -1; h_lmask[b] = 1; }
                }
                HIP_CHECK(hipMemcpyAsync(d_slots.p, h_slots, sizeof(int) * n_entries, hipMemcpyHostToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(d_lmask.p, h_lmask, sizeof(int) * n_entries, hipMemcpyHostToDevice, stream));
                HIP_CHECK(hipMemsetAsync(d_change.p, 0, sizeof(double) * n_slots, stream));
                iter_T = it_total;
                snapshots_before_iteration(active, it + 1);
                if (host_prof) { HIP_CHECK(hipStreamSynchronize(stream)); hp_mark("snapshots"); }
                stamps_ok = (it == 0 ? true : stamps_ok) && stamps_live_for(n_entries);   // (per stage: the stamps are rewritten between the stages)
                h_iter[0] = it_total;
                h_iter[1] = (int)launch_epoch;   // epoch of this iteration's (first) sweep launch
                launch_epoch += (persistent_now() && mode == 2) ? 1u : (unsigned)ndir;
                HIP_CHECK(hipMemcpyAsync(d_iter.p, h_iter, 2 * sizeof(int), hipMemcpyHostToDevice, stream));
                // first launch of the call: the spare set -- the results of the call before, which nothing enqueued after the swap reads,
                // the invariant of the side-stream fill below -- is re-initialised by this launch's units; later launches carry no fill
                fill_arm = it_total == 0 && all_slots && !alt_filled && inline_fill_now(n_entries);
                run_iteration(n_entries);
                fill_arm = false;
                HIP_CHECK(hipMemcpyAsync(h_change, d_change.p, sizeof(double) * n_slots, hipMemcpyDeviceToHost, stream));
                if (persistent_now()) HIP_CHECK(hipMemcpyAsync(h_abort, d_sync.p + 4, sizeof(int), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
                hp_mark("sweep-iteration");
                if (persistent_now() && *h_abort) {
                    HIP_CHECK(hipMemsetAsync(d_sync.p + 4, 0, sizeof(int), stream));
                    stage = 0;
                    throw DeviceError("persistent sweep kernel: a patch timed out waiting for its upwind neighbour");
                }
                if (fill_in_flight) { inline_filled = true; fill_in_flight = false; }   // (synchronised, not aborted: every ticket was drawn)
                ++it;
                ++it_total;
                std::vector<int> next;
                if (fixed_iters > 0) ref_change_last.assign(n_slots, std::nan(""));
                const std::vector<char> go = fixed_iters > 0 ? std::vector<char>(active.size(), 1) : decide_go_on(active, it);
                hp_mark("stopping rule");
                for (size_t q = 0; q < active.size(); ++q) {
                    const int s2 = active[q];
                    (stage == 0 ? niter : niterw)[s2] = it;
                    (stage == 0 ? change_hist : change_histw)[s2].push_back(h_change[s2]);
                    (stage == 0 ? ref_hist : ref_histw)[s2].push_back((int)ref_change_last.size() == n_slots ? ref_change_last[s2] : std::nan(""));
                    timing.node_updates += (long long)n_nodes * ndir;
                    prev2_change[s2] = prev_change[s2];
                    prev_change[s2] = h_change[s2];
                    if (go[q]) next.push_back(s2);
                }
                active.swap(next);
            }
            timing.iterations = std::max(timing.iterations, it_total);
            // the stamps of the first-order stage say nothing about the WENO stencil: every brick counts as changed in the
            // last sweep, so that the first WENO sweep visits every node once with the new formula
            if (stage == 0 && weno) {
                // (and no whole-sweep shortcut across the stage boundary: a tally of zero finished units never qualifies)
                HIP_CHECK(hipMemsetAsync(d_sw.p, 0, sizeof(unsigned long long) * (size_t)sw_sweeps * n_groups(), stream));
                for (int s2 : slot_ids)
                    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(d_stamp.p + (size_t)(s2 / NS) * n_bricks), it_total * (dim == 3 ? 8 : 4),
                                                n_bricks, stream));
            }
        }
        if (std::getenv("TTCR_FSM_DEBUG_SW")) {   // tuning: the whole-sweep tallies of the SKIP kernels
            std::vector<unsigned long long> h((size_t)std::min(sw_sweeps, 40) * n_groups());
            HIP_CHECK(hipMemcpy(h.data(), d_sw.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < h.size(); ++q) std::fprintf(stderr, "%s%u/%u", q % n_groups() == 0 ? "\n[sw] " : " ", (unsigned)h[q], (unsigned)(h[q] >> 32));
            std::fprintf(stderr, "\n");
        }
        const bool was_persistent = mode >= 1 || weno;
        stage = 0;
        sync_clean = true;
        HIP_CHECK(hipEventRecord(ev1, stream));
        if (all_slots && inline_filled) {
            alt_filled = true;   // (complete since the first launch: ev_fill, long signalled, has nothing to add)
            ++prefill_inline_fills;
        } else if (all_slots) {
            // the other set of fields -- fresh, or the results of the call before this one, which nothing enqueued after the swap reads --
            // is initialised for the next call BEHIND this call's sweeps (the event just recorded): beside them the fill took
            // workgroup slots and bandwidth from the sweep kernel and was not done when the next call came (512^3 x 64 back to back:
            // 191.8 ms per step instead of 185.7, profiles/r05/README.md); behind them it runs beside the receiver interpolation and
            // whatever the caller does between two calls, and a call that comes at once waits for what is left of it
            const size_t n_el = n_nodes * tt_fields();   // (room for either layout)
            if (!fill_stream) {
                int lo = 0, hi = 0;
                HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
                HIP_CHECK(hipStreamCreateWithPriority(&fill_stream, hipStreamNonBlocking, lo));
                HIP_CHECK(hipEventCreateWithFlags(&ev_fill, hipEventDisableTiming));
            }
            // (a second set of fields is a convenience: when the device has no room for it -- the snapshots of this solve were not
            // there yet when prefill_on() looked -- the solve that just finished must not fail for it)
            bool have_alt = true;
            try {
                d_tt_alt.reserve(n_el, 64);
            } catch (const DeviceError&) {
                (void)hipGetLastError();
                have_alt = false;
                prefill = 0;
            }
            if (have_alt) {
            HIP_CHECK(hipStreamWaitEvent(fill_stream, ev1, 0));
            const int blocks = (int)std::min<size_t>((n_el + 255) / 256, 16384);
            fsm_fill<T><<<blocks, 256, 0, fill_stream>>>(d_tt_alt.p, n_el, real_traits<T>::max(), 1);
            HIP_CHECK(hipEventRecord(ev_fill, fill_stream));
            alt_filled = true;
            }
        }
        HIP_CHECK(hipEventSynchronize(ev1));
        if (d_prof.p) {
            unsigned long long h[8];
            HIP_CHECK(hipMemcpy(h, d_prof.p, sizeof(h), hipMemcpyDeviceToHost));
            if (const char* tp = std::getenv("TTCR_FSM_PROF_TRACE")) {   // unit trace of the last iteration -> file
                std::vector<unsigned long long> tr(prof_words);
                HIP_CHECK(hipMemcpy(tr.data(), d_prof.p, prof_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                if (FILE* f = std::fopen(tp, "wb")) { std::fwrite(tr.data() + 8, sizeof(unsigned long long), prof_words - 8, f); std::fclose(f); }
            }
            HIP_CHECK(hipMemset(d_prof.p, 0, sizeof(h)));
            if (mode >= 1) {
                const double nb_ = (double)std::max<unsigned long long>(h[7], 1), nu_ = (double)std::max<unsigned long long>(h[6], 1);
                std::fprintf(stderr, "[ttcr_amd prof] units %llu chunks %llu  per unit (us): start %.2f total %.2f | per chunk (us): top %.3f  wait %.3f  stage %.3f  march %.3f  writeback %.3f\n",
                             h[6], h[7], h[5] * 0.01 / nu_, (h[0] + h[1] + h[2] + h[3] + h[4] + h[5]) * 0.01 / nu_, h[0] * 0.01 / nb_,
                             h[1] * 0.01 / nb_, h[2] * 0.01 / nb_, h[3] * 0.01 / nb_, h[4] * 0.01 / nb_);
            } else {
                const double nb_ = (double)std::max<unsigned long long>(h[4], 1);
                std::fprintf(stderr, "[ttcr_amd prof] tiles %llu  per tile (us): setup %.2f  stage %.2f  march %.2f  writeback %.2f\n",
                             h[4], h[0] * 0.01 / nb_, h[1] * 0.01 / nb_, h[2] * 0.01 / nb_, h[3] * 0.01 / nb_);
            }
        }
        hp_mark("after the iterations");
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        timing.sweep_ms += ms;
        const long long evaluated_before = timing.evaluated_updates;
        if (was_persistent) {
            HIP_CHECK(hipMemcpy(h_evals, d_evals.p, sizeof(unsigned long long) * n_slots, hipMemcpyDeviceToHost));
            for (int s2 : slot_ids) timing.evaluated_updates += (long long)h_evals[s2];
        } else {
            timing.evaluated_updates += timing.node_updates - node_updates_before;   // every update is evaluated
        }
        const bool skipped_now = skip_now(n_groups());
        if (nb == n_slots && timing.node_updates > node_updates_before && skipped_now)   // (what choose_layout goes by; kernels that skip only)
            last_eval_frac = (double)(timing.evaluated_updates - evaluated_before) / (double)(timing.node_updates - node_updates_before);
        if (skip < 0 && !weno && fsm_in_probe_window(facts((nb + NS - 1) / NS), tune) && timing.node_updates > node_updates_before) {   // (see skip_probe_min)
            if (skipped_now) {
                probe_skip = (double)(timing.evaluated_updates - evaluated_before) / (double)(timing.node_updates - node_updates_before) < 0.6;
                probe_off_calls = 0;
            } else if (++probe_off_calls >= 8) {
                probe_skip = true;
                probe_off_calls = 0;
            }
        }
    }

    void interp(int slot, int n, const void* pts, void* out) override {
        HIP_CHECK(hipSetDevice(device));
        check_slot(slot);
        if (n <= 0) return;
        const int nc = ncoord();
        std::vector<T> p((const T*)pts, (const T*)pts + (size_t)nc * n);
        if (translate)
            for (int m = 0; m < n; ++m) { p[3 * m] -= ox; p[3 * m + 1] -= oy; p[3 * m + 2] -= oz; }
        check_pts(p.data(), n);
        interp_grid_coords(P(slot), n, p.data(), (T*)out);
    }

    // Grid3Drn::computeSlowness(pt, isTranslated) (ttcr/Grid3Drn.h:2451-2676), Grid2Drn::computeSlowness (ttcr/Grid2Drn.h:262-330)
    void compute_slowness(int n, const void* pts, bool translated, void* out) override {
        HIP_CHECK(hipSetDevice(device));
        if (!have_slowness) throw std::runtime_error("Error: slowness has not been assigned.");
        if (n <= 0) return;
        const int nc = ncoord();
        std::vector<T> p((const T*)pts, (const T*)pts + (size_t)nc * n);
        if (translate && !translated)
            for (int m = 0; m < n; ++m) { p[3 * m] -= ox; p[3 * m + 1] -= oy; p[3 * m + 2] -= oz; }
        check_pts(p.data(), n);   // (the reference indexes its node array unchecked; a point outside is refused here)
        d_rx.reserve((size_t)nc * n);
        d_out.reserve(n);
        HIP_CHECK(hipMemcpyAsync(d_rx.p, p.data(), sizeof(T) * nc * n, hipMemcpyHostToDevice, stream));
        const int blocks = (n + 63) / 64;
        if (dim == 3) {
            RayGeom<T> rg;
            rg.nnx = ncx + 1; rg.nny = ncy + 1; rg.nnz = ncz + 1;
            rg.dx = dx; rg.xmin = xmin; rg.ymin = ymin; rg.zmin = zmin; rg.xmax = xmax; rg.ymax = ymax; rg.zmax = zmax;
            rg.interp_vel = interp_vel;
            fsm_compute_slowness3d<T><<<blocks, 64, 0, stream>>>(rg, d_s.p, d_rx.p, n, d_out.p);
        } else {
            RayGeom2<T> rg2;
            rg2.nnx = ncx + 1; rg2.nnz = ncz + 1;
            rg2.dx = dx; rg2.dz = dz; rg2.xmin = xmin; rg2.zmin = zmin; rg2.xmax = xmax; rg2.zmax = zmax;
            fsm_compute_slowness2d<T><<<blocks, 64, 0, stream>>>(rg2, d_s.p, d_rx.p, n, d_out.p);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, d_out.p, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    void interp_grid_coords(int slot, int n, const T* p, T* out) {
        if (n <= 0) return;
        const int nc = ncoord();
        d_rx.reserve((size_t)nc * n);
        d_out.reserve(n);
        HIP_CHECK(hipMemcpyAsync(d_rx.p, p, sizeof(T) * nc * n, hipMemcpyHostToDevice, stream));
        const T* tt = tt_ptr(slot);
        const int blocks = (n + 127) / 128;
        if (dim == 3)
            fsm_interp3d<T><<<blocks, 128, 0, stream>>>(tt, NS, d_rx.p, d_out.p, n, (int)ncx + 1, (int)ncy + 1, (int)ncz + 1, dx, xmin, ymin, zmin);
        else
            fsm_interp2d<T><<<blocks, 128, 0, stream>>>(tt, NS, d_rx.p, d_out.p, n, (int)ncx + 1, (int)ncz + 1, dx, dz, xmin, zmin);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, d_out.p, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // the same for every source of a batch: one upload, one launch, one read-back
    void interp_batch(const std::vector<int>& sl, const std::vector<int>& sr, const int* rx_off, const T* rx, T* tt_out) {
        const int nc = ncoord();
        size_t n = 0;
        for (int s2 : sr) n += (size_t)(rx_off[s2 + 1] - rx_off[s2]);
        if (n == 0) return;
        std::vector<T> p(nc * n), o(n);
        std::vector<int> so(n);
        size_t k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int m = rx_off[sr[b] + 1] - rx_off[sr[b]];
            std::memcpy(p.data() + nc * k, rx + (size_t)nc * rx_off[sr[b]], sizeof(T) * nc * m);
            std::fill(so.begin() + k, so.begin() + k + m, sl[b]);
            k += m;
        }
        d_rx.reserve(nc * n);
        d_out.reserve(n);
        d_rslot.reserve(n);
        HIP_CHECK(hipMemcpyAsync(d_rx.p, p.data(), sizeof(T) * nc * n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rslot.p, so.data(), sizeof(int) * n, hipMemcpyHostToDevice, stream));
        const int blocks = (int)((n + 127) / 128);
        if (dim == 3)
            fsm_interp3d_batch<T><<<blocks, 128, 0, stream>>>(d_tt.p, NS, n_nodes, d_rslot.p, d_rx.p, d_out.p, (int)n, (int)ncx + 1,
                                                              (int)ncy + 1, (int)ncz + 1, dx, xmin, ymin, zmin);
        else
            fsm_interp2d_batch<T><<<blocks, 128, 0, stream>>>(d_tt.p, NS, n_nodes, d_rslot.p, d_rx.p, d_out.p, (int)n, (int)ncx + 1, (int)ncz + 1, dx,
                                                              dz, xmin, zmin);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(o.data(), d_out.p, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int m = rx_off[sr[b] + 1] - rx_off[sr[b]];
            std::memcpy(tt_out + rx_off[sr[b]], o.data() + k, sizeof(T) * m);
            k += m;
        }
    }

    // a walk that failed on the device -> the reference's exception (ttcr/Grid3Drn.h:1170-1181); status 2 is our
    // step limit, where the reference would not return
    [[noreturn]] void throw_walk_error(int st, const T* rx, const T* tx, long max_steps) const {
        const int nc = ncoord();
        std::ostringstream msg;
        auto pt = [&](const T* v) { for (int c = 0; c < nc; ++c) msg << (c ? " " : "") << v[c]; };
        if (st == 1) {
            msg << "Error while computing raypaths: going outside grid \n                Rx: ";
            pt(rx);
            msg << "\n                Tx: ";
            pt(tx);
            msg << "\n";
        } else {
            msg << "Error while computing raypaths: ray from Rx ";
            pt(rx);
            msg << " did not reach the source within " << max_steps << " steps";
        }
        throw std::runtime_error(msg.str());
    }

    // getTraveltimeFromRaypath for the receivers of every source of a batch in ONE launch (one thread per receiver:
    // a single source's few hundred receivers leave the device empty); errors as in raypath_batch_rays
    void raypath_batch(const std::vector<int>& sl, const std::vector<int>& sr, const int* tx_off, const T* tx, const T* t0,
                       const int* rx_off, const T* rx, T* tt_out) {
        const int nc = ncoord();
        size_t n = 0;
        for (int s2 : sr) n += (size_t)(rx_off[s2 + 1] - rx_off[s2]);
        if (n == 0) return;
        std::vector<T> p(nc * n), o(n), txb;
        std::vector<T> t0b;
        std::vector<int> so(n), st(n);
        std::vector<RaySrc> desc(sl.size());
        size_t k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int src = sr[b], m = rx_off[src + 1] - rx_off[src];
            desc[b].tt_off = (long long)(tt_ptr(sl[b]) - d_tt.p);
            desc[b].tx_off = (int)t0b.size();
            desc[b].n_tx = tx_off[src + 1] - tx_off[src];
            txb.insert(txb.end(), tx + (size_t)nc * tx_off[src], tx + (size_t)nc * tx_off[src + 1]);
            t0b.insert(t0b.end(), t0 + tx_off[src], t0 + tx_off[src + 1]);
            std::memcpy(p.data() + nc * k, rx + (size_t)nc * rx_off[src], sizeof(T) * nc * m);
            std::fill(so.begin() + k, so.begin() + k + m, (int)b);
            k += m;
        }
        d_rsrc.reserve(txb.size());
        d_rt0.reserve(t0b.size());
        d_rx.reserve(nc * n);
        d_out.reserve(n);
        d_rstat.reserve(n);
        d_rslot.reserve(n);
        d_rdesc.reserve(desc.size());
        HIP_CHECK(hipMemcpyAsync(d_rsrc.p, txb.data(), sizeof(T) * txb.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rt0.p, t0b.data(), sizeof(T) * t0b.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rx.p, p.data(), sizeof(T) * nc * n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rslot.p, so.data(), sizeof(int) * n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rdesc.p, desc.data(), sizeof(RaySrc) * desc.size(), hipMemcpyHostToDevice, stream));
        const long max_steps = walk_step_limit;
        const dim3 rgrid((unsigned)((n + 63) / 64)), rblock(64);
        if (dim == 3) {
            RayGeom<T> rg;
            rg.nnx = ncx + 1; rg.nny = ncy + 1; rg.nnz = ncz + 1;
            rg.dx = dx; rg.xmin = xmin; rg.ymin = ymin; rg.zmin = zmin; rg.xmax = xmax; rg.ymax = ymax; rg.zmax = zmax;
            rg.interp_vel = interp_vel;
            fsm_raypath3d<T, false><<<rgrid, rblock, 0, stream>>>(d_tt.p, NS, d_s.p, rg, 0, d_rsrc.p, d_rt0.p, d_rx.p, (int)n, d_out.p,
                                                                  d_rstat.p, max_steps, nullptr, 0, nullptr, d_rdesc.p, d_rslot.p);
        } else {
            RayGeom2<T> rg2;
            rg2.nnx = ncx + 1; rg2.nnz = ncz + 1;
            rg2.dx = dx; rg2.dz = dz; rg2.xmin = xmin; rg2.zmin = zmin; rg2.xmax = xmax; rg2.zmax = zmax;
            const T* cell_s = cell ? d_cells.p : nullptr;
            fsm_raypath2d<T, false><<<rgrid, rblock, 0, stream>>>(d_tt.p, NS, d_s.p, cell_s, rg2, 0, d_rsrc.p, d_rt0.p, d_rx.p, (int)n,
                                                                  d_out.p, d_rstat.p, max_steps, nullptr, 0, nullptr, d_rdesc.p, d_rslot.p);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(o.data(), d_out.p, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(st.data(), d_rstat.p, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        for (size_t q = 0; q < n; ++q)
            if (st[q] != 0) throw_walk_error(st[q], p.data() + (size_t)nc * q, txb.data() + (size_t)nc * desc[so[q]].tx_off, max_steps);
        k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int m = rx_off[sr[b] + 1] - rx_off[sr[b]];
            std::memcpy(tt_out + rx_off[sr[b]], o.data() + k, sizeof(T) * m);
            k += m;
        }
    }

    // getRaypath (the r_data overloads, ttcr/Grid3D.h:546-586 / Grid2D) for the receivers of every source of a batch in ONE launch
    // per chunk of rows: a walk is a chain of dependent loads (≈ 10 ms for ANY number of receivers of a 256^3 source), so one
    // launch per source made a call with return_rays cost more than its solves.  Rows in batch order; recording rows hold the
    // length of an ordinary ray, a longer one is traced again alone; the recording buffer stays below rays_buffer_bytes.
    size_t rays_buffer_bytes = (size_t)4 << 30;
    void raypath_batch_rays(const std::vector<int>& sl, const std::vector<int>& sr, const int* tx_off, const T* tx, const T* t0,
                            const int* rx_off, const T* rx, T* tt_out, std::vector<std::vector<long long>>& src_ray_len,
                            std::vector<std::vector<T>>& src_ray_pts) {
        const int nc = ncoord();
        size_t n = 0;
        for (int s2 : sr) n += (size_t)(rx_off[s2 + 1] - rx_off[s2]);
        if (n == 0) return;
        std::vector<T> p(nc * n), o(n), txb, t0b;
        std::vector<int> so(n), st(n), np(n);
        std::vector<RaySrc> desc(sl.size());
        size_t k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int src = sr[b], m = rx_off[src + 1] - rx_off[src];
            desc[b].tt_off = (long long)(tt_ptr(sl[b]) - d_tt.p);
            desc[b].tx_off = (int)t0b.size();
            desc[b].n_tx = tx_off[src + 1] - tx_off[src];
            txb.insert(txb.end(), tx + (size_t)nc * tx_off[src], tx + (size_t)nc * tx_off[src + 1]);
            t0b.insert(t0b.end(), t0 + tx_off[src], t0 + tx_off[src + 1]);
            std::memcpy(p.data() + nc * k, rx + (size_t)nc * rx_off[src], sizeof(T) * nc * m);
            std::fill(so.begin() + k, so.begin() + k + m, (int)b);
            k += m;
        }
        d_rsrc.reserve(txb.size());
        d_rt0.reserve(t0b.size());
        d_rx.reserve(nc * n);
        d_out.reserve(n);
        d_rstat.reserve(n);
        d_rslot.reserve(n);
        d_raynp.reserve(n);
        d_rdesc.reserve(desc.size());
        HIP_CHECK(hipMemcpyAsync(d_rsrc.p, txb.data(), sizeof(T) * txb.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rt0.p, t0b.data(), sizeof(T) * t0b.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rx.p, p.data(), sizeof(T) * nc * n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rslot.p, so.data(), sizeof(int) * n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rdesc.p, desc.data(), sizeof(RaySrc) * desc.size(), hipMemcpyHostToDevice, stream));
        RayGeom<T> rg;
        rg.nnx = ncx + 1; rg.nny = ncy + 1; rg.nnz = ncz + 1;
        rg.dx = dx; rg.xmin = xmin; rg.ymin = ymin; rg.zmin = zmin; rg.xmax = xmax; rg.ymax = ymax; rg.zmax = zmax;
        rg.interp_vel = interp_vel;
        RayGeom2<T> rg2;
        rg2.nnx = ncx + 1; rg2.nnz = ncz + 1;
        rg2.dx = dx; rg2.dz = dz; rg2.xmin = xmin; rg2.zmin = zmin; rg2.xmax = xmax; rg2.zmax = zmax;
        const T* cell_s = (dim == 2 && cell) ? d_cells.p : nullptr;
        // The reference's walk has no step limit: next to a corner it can go back and forth between two planes for tens of thousands
        // of steps before it drifts away (41 512 points for a receiver 1.7e-4 inside the far corner of a 2-D cell grid,
        // tests/test_parity_gpu.py).  The limit only turns a walk that would never end into an error.
        const long max_steps = walk_step_limit;
        const long cap = walk_room(8L * ((long)ncx + ncy + ncz + 3)) + 3;   // Rx, one point per step, <= two per source point
        // (the recording rows of a launch: at most rays_buffer_bytes, and at most a quarter of what the device has free -- a replica that is
        // full of slots, or a smaller device, records in more launches instead of failing its allocation)
        size_t rays_budget = rays_buffer_bytes, free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) rays_budget = std::min(rays_budget, std::max<size_t>(free_b / 4, (size_t)64 << 20));
        const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, rays_budget / (sizeof(T) * nc * cap)));
        auto launch = [&](size_t row0, int m, T* pts, long rcap) {   // rows [row0, row0 + m) of the batch
            const dim3 rgrid((unsigned)((m + 63) / 64)), rblock(64);
            if (dim == 3)
                fsm_raypath3d<T, true><<<rgrid, rblock, 0, stream>>>(d_tt.p, NS, d_s.p, rg, 0, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)nc * row0, m,
                                                                     d_out.p + row0, d_rstat.p + row0, max_steps, pts, rcap, d_raynp.p + row0,
                                                                     d_rdesc.p, d_rslot.p + row0);
            else
                fsm_raypath2d<T, true><<<rgrid, rblock, 0, stream>>>(d_tt.p, NS, d_s.p, cell_s, rg2, 0, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)nc * row0, m,
                                                                     d_out.p + row0, d_rstat.p + row0, max_steps, pts, rcap, d_raynp.p + row0,
                                                                     d_rdesc.p, d_rslot.p + row0);
            HIP_CHECK(hipGetLastError());
        };
        auto compact = [&](const T* pts, long rcap, const long long* d_off, int m) {
            if (dim == 3)
                fsm_compact_rays<T><<<m, 128, 0, stream>>>(pts, rcap, d_off, d_raydense.p, shift_rays() ? ox : (T)0, shift_rays() ? oy : (T)0,
                                                           shift_rays() ? oz : (T)0);
            else
                fsm_compact_rays2<T><<<m, 128, 0, stream>>>(pts, rcap, d_off, d_raydense.p);
            HIP_CHECK(hipGetLastError());
        };
        std::vector<long long> off;
        std::vector<T> dense;
        for (size_t c0 = 0; c0 < n; c0 += chunk) {
            const int m = (int)std::min(chunk, n - c0);
            d_raypts.reserve((size_t)m * cap * nc);
            launch(c0, m, d_raypts.p, cap);
            HIP_CHECK(hipMemcpyAsync(o.data() + c0, d_out.p + c0, sizeof(T) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(st.data() + c0, d_rstat.p + c0, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(np.data() + c0, d_raynp.p + c0, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            for (int q = 0; q < m; ++q)
                if (st[c0 + q] != 0 && st[c0 + q] != 3)
                    throw_walk_error(st[c0 + q], p.data() + (size_t)nc * (c0 + q), txb.data() + (size_t)nc * desc[so[c0 + q]].tx_off, max_steps);
            off.assign((size_t)m + 1, 0);
            for (int q = 0; q < m; ++q) off[q + 1] = off[q] + np[c0 + q];
            const long long tot = off[m];
            d_rayoff.reserve((size_t)m + 1);
            d_raydense.reserve((size_t)std::max<long long>(tot, 1) * nc);
            HIP_CHECK(hipMemcpyAsync(d_rayoff.p, off.data(), sizeof(long long) * ((size_t)m + 1), hipMemcpyHostToDevice, stream));
            compact(d_raypts.p, cap, d_rayoff.p, m);
            for (int q = 0; q < m; ++q) {   // rays longer than a row (status 3): once more, alone, with room
                if (st[c0 + q] != 3) continue;
                const long need = (long)np[c0 + q] + 1;
                d_raylong.reserve((size_t)need * nc);
                const long long off2[2] = {off[q], off[q + 1]};
                d_rayoff2.reserve(2);
                HIP_CHECK(hipMemcpyAsync(d_rayoff2.p, off2, sizeof(off2), hipMemcpyHostToDevice, stream));
                launch(c0 + q, 1, d_raylong.p, need);
                compact(d_raylong.p, need, d_rayoff2.p, 1);
                int st2 = 0, np2 = 0;
                HIP_CHECK(hipMemcpyAsync(&st2, d_rstat.p + c0 + q, sizeof(int), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipMemcpyAsync(&np2, d_raynp.p + c0 + q, sizeof(int), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipMemcpyAsync(o.data() + c0 + q, d_out.p + c0 + q, sizeof(T), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));   // (also: off2 goes out of scope)
                if (st2 != 0 || np2 != np[c0 + q]) throw DeviceError("raypath: a long ray did not retrace to the same length");
            }
            dense.resize((size_t)tot * nc);
            if (tot > 0) HIP_CHECK(hipMemcpyAsync(dense.data(), d_raydense.p, sizeof(T) * nc * tot, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            for (int q = 0; q < m; ++q) {   // hand the rays to their sources (rows of a source are consecutive)
                const int src = sr[so[c0 + q]];
                src_ray_len[src].push_back((long long)np[c0 + q]);
                src_ray_pts[src].insert(src_ray_pts[src].end(), dense.begin() + (size_t)off[q] * nc, dense.begin() + (size_t)off[q + 1] * nc);
            }
        }
        k = 0;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int m = rx_off[sr[b] + 1] - rx_off[sr[b]];
            std::memcpy(tt_out + rx_off[sr[b]], o.data() + k, sizeof(T) * m);
            k += m;
        }
    }

    // rays of the last raytrace call with return_rays on, in the order of the receiver rows of that call
    std::vector<long long> rays_off{0};
    std::vector<T> rays_pts;
    DevBuf<T> d_raypts, d_raydense, d_raylong;
    DevBuf<long long> d_rayoff2;
    DevBuf<int> d_raynp;
    DevBuf<long long> d_rayoff;

    bool shift_rays() const { return translate; }

    // ---- matrix M (the raytrace overloads with m_data: ttcr/Grid3D.h:743-772 -> Grid3Drn::getRaypath(Tx, t0, Rx, m_data, RxNo, tt,
    // threadNo), ttcr/Grid3Drn.h:1503-1800; with r_data as well, what ttcrpy calls for compute_M with return_rays:
    // ttcr/Grid3D.h:646-680 -> getRaypath(Tx, t0, Rx, r_data, m_data, RxNo, tt, threadNo), ttcr/Grid3Drn.h:2144-2470).  The walk
    // of either overload is a kernel of its own (fsm_raypath3d_m) that leaves one record (mid-point, length, slowness at the
    // mid-point) per term block of the reference; the host adds -s^2 * ds * w at the eight nodes around each mid-point.
    // Restated as it stands (weights without xmin, node indices that may lie one past the grid -- the Python layer drops those;
    // the zero-length segments of the m_data-only overload give signed zeros), entries merged by node in push order; a receiver
    // on the source: no entries and tt = 0, not t0.
    std::vector<std::vector<long long>> slot_m_off, slot_m_j;
    std::vector<std::vector<T>> slot_m_v;
    DevBuf<T> d_msegs, d_mlong;
    DevBuf<int> d_mnseg;
    // records of every receiver's walk: seg_off[q] .. seg_off[q+1] in segs (5 values each), traveltimes of the overload in out
    // sink (the M tape): the records stay on the device and are merged there into (row_base + receiver, node, value) entries appended
    // to *sink, chunk by chunk (fsm_tape_api.h); segs stays empty
    TapeChunk m_chunk;
    void walk_m(int slot, int n_tx, const T* txp, const T* t0p, int n, const T* p, T* out, bool both, std::vector<long long>& seg_off,
                std::vector<T>& segs, TapeRows* sink = nullptr, int row_base = 0) {
        seg_off.assign(1, 0);
        segs.clear();
        if (n <= 0) return;
        d_rsrc.reserve((size_t)3 * n_tx);
        d_rt0.reserve(n_tx);
        HIP_CHECK(hipMemcpyAsync(d_rsrc.p, txp, sizeof(T) * 3 * n_tx, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rt0.p, t0p, sizeof(T) * n_tx, hipMemcpyHostToDevice, stream));
        RayGeom<T> rg;
        rg.nnx = ncx + 1; rg.nny = ncy + 1; rg.nnz = ncz + 1;
        rg.dx = dx; rg.xmin = xmin; rg.ymin = ymin; rg.zmin = zmin; rg.xmax = xmax; rg.ymax = ymax; rg.zmax = zmax;
        rg.interp_vel = interp_vel;
        const long max_steps = walk_step_limit;
        // one record per step, up to two per source point at the end; a longer walk is done again with the room it asked for
        const long cap = walk_room(8L * ((long)ncx + ncy + ncz + 3)) + 2L * n_tx + 1;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (sizeof(T) * 5 * cap)));
        std::vector<int> st(chunk), ns(chunk);
        std::vector<T> rows;
        for (int c0 = 0; c0 < n; c0 += chunk) {
            const int m = std::min(chunk, n - c0);
            const T* pc = p + (size_t)3 * c0;
            d_rx.reserve((size_t)3 * m);
            d_out.reserve(m);
            d_rstat.reserve(m);
            d_msegs.reserve((size_t)m * cap * 5);
            d_mnseg.reserve(m);
            HIP_CHECK(hipMemcpyAsync(d_rx.p, pc, sizeof(T) * 3 * m, hipMemcpyHostToDevice, stream));
            const dim3 rgrid((m + 63) / 64), rblock(64);
            if (both)
                fsm_raypath3d_m<T, true><<<rgrid, rblock, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p, m, d_out.p,
                                                                       d_rstat.p, max_steps, d_msegs.p, cap, d_mnseg.p);
            else
                fsm_raypath3d_m<T, false><<<rgrid, rblock, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p, m, d_out.p,
                                                                        d_rstat.p, max_steps, d_msegs.p, cap, d_mnseg.p);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(out + c0, d_out.p, sizeof(T) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(st.data(), d_rstat.p, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(ns.data(), d_mnseg.p, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            for (int q = 0; q < m; ++q)
                if (st[q] != 0 && st[q] != 3) throw_walk_error(st[q], pc + (size_t)3 * q, txp, max_steps);
            if (sink) {
                walk_m_to_tape(slot, n_tx, rg, m, cap, st, ns, both, max_steps, *sink, row_base + c0);
                for (int q = 0; q < m; ++q) seg_off.push_back(seg_off.back() + ns[q]);
                continue;
            }
            size_t base = segs.size(), tot = 0;
            for (int q = 0; q < m; ++q) tot += (size_t)5 * ns[q];
            segs.resize(base + tot);   // (once per chunk: the copies below are asynchronous)
            for (int q = 0; q < m; ++q) {
                if (st[q] == 0) {
                    if (ns[q] > 0)
                        HIP_CHECK(hipMemcpyAsync(segs.data() + base, d_msegs.p + (size_t)q * cap * 5, sizeof(T) * 5 * ns[q], hipMemcpyDeviceToHost, stream));
                } else {   // status 3: once more, alone, with room
                    const long need = (long)ns[q] + 1;
                    d_mlong.reserve((size_t)need * 5);
                    if (both)
                        fsm_raypath3d_m<T, true><<<1, 64, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)3 * q, 1,
                                                                       d_out.p + q, d_rstat.p + q, max_steps, d_mlong.p, need, d_mnseg.p + q);
                    else
                        fsm_raypath3d_m<T, false><<<1, 64, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)3 * q, 1,
                                                                        d_out.p + q, d_rstat.p + q, max_steps, d_mlong.p, need, d_mnseg.p + q);
                    HIP_CHECK(hipGetLastError());
                    int st2 = 0, ns2 = 0;
                    HIP_CHECK(hipMemcpyAsync(&st2, d_rstat.p + q, sizeof(int), hipMemcpyDeviceToHost, stream));
                    HIP_CHECK(hipMemcpyAsync(&ns2, d_mnseg.p + q, sizeof(int), hipMemcpyDeviceToHost, stream));
                    HIP_CHECK(hipMemcpyAsync(segs.data() + base, d_mlong.p, sizeof(T) * 5 * ns[q], hipMemcpyDeviceToHost, stream));
                    HIP_CHECK(hipStreamSynchronize(stream));
                    if (st2 != 0 || ns2 != ns[q]) throw DeviceError("compute_M: a long walk did not retrace to the same length");
                }
                base += (size_t)5 * ns[q];
                seg_off.push_back(seg_off.back() + ns[q]);
            }
            HIP_CHECK(hipStreamSynchronize(stream));
        }
    }
    // one chunk of walk_m into the tape: the records of the walks that fitted are expanded where the walk left them, a long walk (status 3)
    // is walked again alone with room and expanded from there, then the chunk's contributions are merged
    void walk_m_to_tape(int slot, int n_tx, const RayGeom<T>& rg, int m, long cap, const std::vector<int>& st, const std::vector<int>& ns,
                        bool both, long max_steps, TapeRows& sink, int row_base) {
        std::vector<long long> roff(m + 1, 0);
        for (int q = 0; q < m; ++q) roff[q + 1] = roff[q] + ns[q];
        MGeom<T> mg{xmin, ymin, zmin, dx, (size_t)ncx + 1, (size_t)ncy + 1, n_nodes};
        m_chunk.begin(roff.data(), m, sizeof(T), stream);
        m_chunk.expand<T>(d_msegs.p, cap, d_rstat.p, 0, m, mg, stream);
        for (int q = 0; q < m; ++q) {
            if (st[q] != 3) continue;
            const long need = (long)ns[q] + 1;
            d_mlong.reserve((size_t)need * 5);
            if (both)
                fsm_raypath3d_m<T, true><<<1, 64, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)3 * q, 1,
                                                               d_out.p + q, d_rstat.p + q, max_steps, d_mlong.p, need, d_mnseg.p + q);
            else
                fsm_raypath3d_m<T, false><<<1, 64, 0, stream>>>(tt_ptr(slot), NS, d_s.p, rg, n_tx, d_rsrc.p, d_rt0.p, d_rx.p + (size_t)3 * q, 1,
                                                                d_out.p + q, d_rstat.p + q, max_steps, d_mlong.p, need, d_mnseg.p + q);
            HIP_CHECK(hipGetLastError());
            int st2 = 0, ns2 = 0;
            HIP_CHECK(hipMemcpyAsync(&st2, d_rstat.p + q, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(&ns2, d_mnseg.p + q, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            if (st2 != 0 || ns2 != ns[q]) throw DeviceError("compute_M: a long walk did not retrace to the same length");
            m_chunk.expand<T>(d_mlong.p, need, d_rstat.p, q, 1, mg, stream);
        }
        m_chunk.merge<T>(row_base, mg, sink, stream);
    }
    // rows of M from the records of walk_m: appended to (mo, mj, mv); mo ends with the running entry count
    void assemble_m(int n_rx, const std::vector<long long>& seg_off, const std::vector<T>& segs, std::vector<long long>& mo,
                    std::vector<long long>& mj, std::vector<T>& mv) const {
        const size_t nnx = ncx + 1, nny = ncy + 1;
        for (int r = 0; r < n_rx; ++r) {
            const size_t row0 = mj.size();
            for (long long q = seg_off[r]; q < seg_off[r + 1]; ++q) {
                long long jt[8];
                T vt[8];
                m_record_terms<T>(segs.data() + 5 * (size_t)q, xmin, ymin, zmin, dx, nnx, nny, jt, vt);
                for (int c = 0; c < 8; ++c) {
                    const long long j = jt[c];
                    const T v = vt[c];
                    size_t e = row0;
                    for (; e < mj.size(); ++e)
                        if (mj[e] == j) { mv[e] += v; break; }
                    if (e == mj.size()) { mj.push_back(j); mv.push_back(v); }
                }
            }
            mo.push_back((long long)mj.size());
        }
    }
    // the m_data overloads for every source of a call: the fields are solved in batches like raytrace_multi solves them, the walks
    // follow each batch (Grid3D's multi-source overloads with m_data, ttcr/Grid3D.h:896-1000, which run the single-source overload
    // per source on host threads).  One CSR over all receiver rows of the call, in row order.
    bool m_walk_mode = false, m_walk_both = false;
    std::vector<std::vector<long long>> m_seg_off;
    std::vector<std::vector<T>> m_segs;
    std::vector<long long> multi_m_off{0}, multi_m_j;
    std::vector<T> multi_m_v;
    void raytrace_multi_m(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                          void* tt_out_v, bool both) override {
        if (dim != 3) throw Unsupported("compute_M is implemented for 3-D grids only");
        if (cell) throw Unsupported("compute_M not defined for grids with slowness defined for cells");
        multi_m_off.assign(1, 0); multi_m_j.clear(); multi_m_v.clear();
        if (n_src <= 0) return;
        m_seg_off.assign(n_src, std::vector<long long>{0});
        m_segs.assign(n_src, std::vector<T>());
        m_walk_mode = true; m_walk_both = both;
        try {
            raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, -1, nullptr, both);
        } catch (...) { m_walk_mode = false; throw; }
        m_walk_mode = false;
        for (int n = 0; n < n_src; ++n) {
            assemble_m(rx_off[n + 1] - rx_off[n], m_seg_off[n], m_segs[n], multi_m_off, multi_m_j, multi_m_v);
            std::vector<T>().swap(m_segs[n]);
        }
    }
    // the M tape: the walks of raytrace_multi_m (without rays), each source's rows merged on the device, then put together in source order
    std::vector<TapeRows> m_tape_src;
    void raytrace_multi_tape(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                             void* tt_out_v, TapeRows& out) override {
        if (dim != 3) throw Unsupported("compute_M is implemented for 3-D grids only");
        if (cell) throw Unsupported("compute_M not defined for grids with slowness defined for cells");
        HIP_CHECK(hipSetDevice(device));
        out.release();
        out.elem = sizeof(T);
        if (n_src <= 0) return;
        m_seg_off.assign(n_src, std::vector<long long>{0});
        m_segs.assign(n_src, std::vector<T>());
        m_tape_src.clear();
        m_tape_src.resize(n_src);
        m_walk_mode = true; m_walk_both = false;
        try {
            raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, -1, nullptr, false);
        } catch (...) { m_walk_mode = false; m_tape_src.clear(); m_chunk.release(); throw; }
        m_walk_mode = false;
        size_t tot = 0;
        for (const TapeRows& r : m_tape_src) tot += r.n;
        out.grow(tot, stream);
        for (TapeRows& r : m_tape_src) {
            if (r.n > 0) {
                HIP_CHECK(hipMemcpyAsync(out.row + out.n, r.row, r.n * sizeof(int), hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(out.col + out.n, r.col, r.n * sizeof(int), hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipMemcpyAsync((T*)out.val + out.n, r.val, r.n * sizeof(T), hipMemcpyDeviceToDevice, stream));
                out.n += r.n;
            }
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        m_tape_src.clear();
        m_chunk.release();
        for (auto& v : m_seg_off) std::vector<long long>().swap(v);
    }
    // ---- the field tape (fsm_adjoint_api.h)
    void adjoint_geometry(int* nn3, double* spacing, TapeWrt wrt) const override {
        const bool wrt_cells = wrt == WRT_CELLS;
        if (dim != 3) throw Unsupported("the adjoint-state gradient is implemented for 3-D grids only");
        if (cell && wrt == WRT_MODEL)
            throw ValueError("a coarse model grid needs a grid with slowness defined at the nodes: this grid has it for cells");
        if (cell && !wrt_cells)
            throw Unsupported("the adjoint-state gradient with respect to node slowness is not implemented for grids with slowness defined for "
                              "cells: ttcr_fsm_raytrace_multi_adjoint_cells gives the gradient with respect to the cells");
        if (!cell && wrt_cells)
            throw ValueError("raytrace_multi_adjoint_cells: the grid has slowness defined at the nodes: use ttcr_fsm_raytrace_multi_adjoint");
        if (weno) throw Unsupported("the adjoint-state gradient is implemented for the first-order solver only (weno = 0)");
        nn3[0] = (int)ncx + 1; nn3[1] = (int)ncy + 1; nn3[2] = (int)ncz + 1;
        *spacing = (double)dx;
    }
    void raytrace_multi_adjoint(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                                void* tt_out_v, AdjSink& sink) override {
        int nn3[3];
        double sp;
        adjoint_geometry(nn3, &sp, sink.cells ? WRT_CELLS : WRT_NODES);
        adj_sink = &sink;
        try {
            raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, -1, nullptr, false);
        } catch (...) { adj_sink = nullptr; throw; }
        adj_sink = nullptr;
    }
    DevBuf<T> d_adj_tmp;
    // after the solves of a batch: field (device to device), frozen nodes as fsm_init_source wrote them, receiver stencils
    void adj_record(const std::vector<int>& sl, const std::vector<int>& sr, const int* tx_off, const T* tx, const T* t0, const int* rx_off,
                    const T* rx) {
        AdjSink& sk = *adj_sink;
        const int nnx = (int)ncx + 1, nny = (int)ncy + 1, nnz = (int)ncz + 1;
        for (size_t b = 0; b < sl.size(); ++b) {
            const int n = sr[b];
            const size_t e = adj_src.empty() ? (size_t)n : (size_t)adj_src[n];
            const size_t row0 = adj_row.empty() ? (size_t)rx_off[n] : (size_t)adj_row[n];
            T* dst = (T*)sk.fields + e * n_nodes;
            if (sk.device == device) {
                adj_copy_field<T>(tt_ptr(sl[b]), NS, dst, n_nodes, stream);
            } else {   // (another device: gathered here, then copied across)
                d_adj_tmp.reserve(n_nodes);
                adj_copy_field<T>(tt_ptr(sl[b]), NS, d_adj_tmp.p, n_nodes, stream);
                HIP_CHECK(hipMemcpyAsync(dst, d_adj_tmp.p, n_nodes * sizeof(T), hipMemcpyDefault, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
            if (e == 0) HIP_CHECK(hipMemcpyAsync(sk.slowness, d_s.p, n_nodes * sizeof(T), hipMemcpyDefault, stream));
            // frozen nodes: the points in order, the later writer wins (fsm_init_source, 3-D branch, first order)
            // (with each node the point that wrote it, counted within the event, and c = (p - x) / d in T, +0 where d = 0: DESIGN.md 6d)
            std::vector<int>& fn = sk.fr_node[e];
            std::vector<double>& fd = sk.fr_d[e];
            std::vector<int>& fp = sk.fr_pt[e];
            std::vector<double>& fc = sk.fr_c[e];
            fn.clear(); fd.clear(); fp.clear(); fc.clear();
            int pt = 0;
            T cx = 0, cy = 0, cz = 0;
            auto put = [&](long long m, T d) {
                size_t q = 0;
                while (q < fn.size() && fn[q] != (int)m) ++q;
                if (q == fn.size()) { fn.push_back((int)m); fd.push_back(0.0); fp.push_back(0); fc.insert(fc.end(), 3, 0.0); }
                fd[q] = (double)d; fp[q] = pt;
                fc[3 * q] = (double)cx; fc[3 * q + 1] = (double)cy; fc[3 * q + 2] = (double)cz;
            };
            for (int q = tx_off[n]; q < tx_off[n + 1]; ++q) {
                const InitPoint<T> p = locate(tx + (size_t)3 * q, t0[q]);
                const int b0 = p.on_node ? -1 : 0;
                pt = q - tx_off[n];
                cx = 0; cy = 0; cz = 0;
                if (p.on_node) put(((long long)p.k * nny + p.j) * nnx + p.i, (T)0);
                for (int kk = p.k + b0; kk <= p.k + 1; ++kk)
                    for (int jj = p.j + b0; jj <= p.j + 1; ++jj)
                        for (int ii = p.i + b0; ii <= p.i + 1; ++ii) {
                            if (ii < 0 || ii >= nnx || jj < 0 || jj >= nny || kk < 0 || kk >= nnz) continue;
                            if (ii == p.i && jj == p.j && kk == p.k) continue;
                            const T x = node_coord_h(xmin, (uint32_t)ii, dx), y = node_coord_h(ymin, (uint32_t)jj, dx), z = node_coord_h(zmin, (uint32_t)kk, dx);
                            const T d2 = (x - p.x) * (x - p.x) + (y - p.y) * (y - p.y) + (z - p.z) * (z - p.z);
                            const T d = (T)std::sqrt((double)d2);
                            const bool zero = d == (T)0;
                            cx = zero ? (T)0 : (T)((T)(p.x - x) / d);
                            cy = zero ? (T)0 : (T)((T)(p.y - y) / d);
                            cz = zero ? (T)0 : (T)((T)(p.z - z) / d);
                            put(((long long)kk * nny + jj) * nnx + ii, d);
                        }
            }
            for (int r = rx_off[n]; r < rx_off[n + 1]; ++r) {
                const size_t row = row0 + (size_t)(r - rx_off[n]);
                long long nd[8];
                T wt[8];
                const int cnt = interp3d_stencil<T>(rx[3 * (size_t)r], rx[3 * (size_t)r + 1], rx[3 * (size_t)r + 2], nnx, nny, nnz, dx, xmin, ymin, zmin, nd, wt);
                sk.st_cnt[row] = cnt;
                sk.st_event[row] = (int)e;
                for (int c = 0; c < cnt; ++c) { sk.st_node[8 * row + c] = nd[c]; sk.st_w[8 * row + c] = (double)wt[c]; }
                for (int c = 0; c < 3; ++c) sk.st_p[3 * row + c] = (double)rx[3 * (size_t)r + c];   // (the point as the solver sees it: 6k)
            }
            if (e == 0) {   // (written once, like the slowness: the replicas of a multi-device grid share the geometry)
                sk.rcv_min[0] = (double)xmin; sk.rcv_min[1] = (double)ymin; sk.rcv_min[2] = (double)zmin;
                sk.rcv_shift[0] = (double)ox; sk.rcv_shift[1] = (double)oy; sk.rcv_shift[2] = (double)oz;
                sk.rcv_max[0] = (double)xmax; sk.rcv_max[1] = (double)ymax; sk.rcv_max[2] = (double)zmax;
            }
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    void multi_m_size(size_t* n_rows, size_t* nnz) const override { *n_rows = multi_m_off.size() - 1; *nnz = multi_m_j.size(); }
    void get_multi_m(long long* row_off, long long* j, void* v) const override {
        std::memcpy(row_off, multi_m_off.data(), multi_m_off.size() * sizeof(long long));
        if (!multi_m_j.empty()) {
            std::memcpy(j, multi_m_j.data(), multi_m_j.size() * sizeof(long long));
            std::memcpy(v, multi_m_v.data(), multi_m_v.size() * sizeof(T));
        }
    }
    void raytrace_m(int slot, int n_tx, const void* tx_v, const void* t0_v, int n_rx, const void* rx_v, void* tt_out_v, bool both) override {
        check_slot(slot);
        if (dim != 3) throw Unsupported("compute_M is implemented for 3-D grids only");
        if (cell) throw Unsupported("compute_M not defined for grids with slowness defined for cells");
        if (n_tx < 1) throw ValueError("every source needs at least one point");
        const int tx_off[2] = {0, n_tx}, rx_off[2] = {0, n_rx};
        // the field of the source (and, for the overload that keeps them, the rays: the points of that overload are those of
        // the r_data overload); the receivers' traveltimes are then replaced by those of the m_data walk
        raytrace_multi(1, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, slot, nullptr, both);
        T* tt_out = (T*)tt_out_v;
        std::vector<T> txs((const T*)tx_v, (const T*)tx_v + 3 * (size_t)n_tx), rxs((const T*)rx_v, (const T*)rx_v + 3 * (size_t)n_rx);
        if (translate) {
            for (int q = 0; q < n_tx; ++q) { txs[3 * q] -= ox; txs[3 * q + 1] -= oy; txs[3 * q + 2] -= oz; }
            for (int q = 0; q < n_rx; ++q) { rxs[3 * q] -= ox; rxs[3 * q + 1] -= oy; rxs[3 * q + 2] -= oz; }
        }
        std::vector<long long> seg_off;
        std::vector<T> segs;
        // (the source was solved in the PHYSICAL slot P(slot) -- pair_sources may have permuted the map in an earlier batched call)
        walk_m(P(slot), n_tx, txs.data(), (const T*)t0_v, n_rx, rxs.data(), tt_out, both, seg_off, segs);
        if (slot_m_off.empty()) { slot_m_off.resize(n_slots); slot_m_j.resize(n_slots); slot_m_v.resize(n_slots); }
        slot_m_off[slot].assign(1, 0); slot_m_j[slot].clear(); slot_m_v[slot].clear();
        assemble_m(n_rx, seg_off, segs, slot_m_off[slot], slot_m_j[slot], slot_m_v[slot]);
        // the rays of the overload that keeps them (already shifted back by the origin of a translated grid)
        if (slot_rays_off.empty()) { slot_rays_off.assign(n_slots, std::vector<long long>{0}); slot_rays_pts.resize(n_slots); }
        if (both) {
            slot_rays_off[slot] = rays_off;
            slot_rays_pts[slot] = rays_pts;
        } else {
            slot_rays_off[slot].assign(1, 0);
            slot_rays_pts[slot].clear();
        }
        rays_off.assign(1, 0);
        rays_pts.clear();
    }
    void slot_m_size(int slot, size_t* n_rows, size_t* nnz) const override {
        check_slot(slot);
        if (slot_m_off.empty() || slot_m_off[slot].empty()) { *n_rows = 0; *nnz = 0; return; }
        *n_rows = slot_m_off[slot].size() - 1;
        *nnz = slot_m_j[slot].size();
    }
    void get_slot_m(int slot, long long* row_off, long long* j, void* v) const override {
        check_slot(slot);
        if (slot_m_off.empty() || slot_m_off[slot].empty()) { row_off[0] = 0; return; }
        std::memcpy(row_off, slot_m_off[slot].data(), slot_m_off[slot].size() * sizeof(long long));
        if (!slot_m_j[slot].empty()) {
            std::memcpy(j, slot_m_j[slot].data(), slot_m_j[slot].size() * sizeof(long long));
            std::memcpy(v, slot_m_v[slot].data(), slot_m_v[slot].size() * sizeof(T));
        }
    }

    // ---- matrix L (the raytrace overloads with l_data, ttcr/Grid2D.h:583-640 -> Grid2Drn::getRaypath(Tx, t0, Rx, [r_data,] l_data,
    // tt, threadNo), ttcr/Grid2Drn.h:1852-2190): per receiver the (cell, length) entries of its ray, sorted by cell with the
    // reference's comparator (CompareSiv_i, ttcr/ttcr_t.h:417-422, std::sort -- entries of one cell keep whatever order that
    // gives them, like in the reference).  The walk is a kernel of its own (fsm_raypath2d_l).
    std::vector<std::vector<long long>> slot_l_off, slot_l_cell;
    std::vector<std::vector<T>> slot_l_val;
    DevBuf<uint32_t> d_lcell;
    DevBuf<T> d_lval;
    DevBuf<int> d_lnum;
    // the walk of the l_data overloads for the receivers of the source whose field lies in `slot`: (cell, length) entries per receiver,
    // sorted like the reference sorts them; the rays of the overload that keeps them
    void walk_l(int slot, int n_tx, const void* tx_v, const void* t0_v, int n_rx, const void* rx_v, void* tt_out_v, bool with_rays,
                std::vector<long long>& loff, std::vector<long long>& lcell, std::vector<T>& lval, std::vector<long long>& roff,
                std::vector<T>& rpts) {
        const int ps = slot;   // (a PHYSICAL slot, like walk_m's: the callers translate)
        loff.assign(1, 0); lcell.clear(); lval.clear();
        roff.assign(1, 0); rpts.clear();
        if (n_rx <= 0) return;
        check_pts((const T*)rx_v, n_rx);
        T* tt_out = (T*)tt_out_v;
        d_rsrc.reserve(2 * (size_t)n_tx);
        d_rt0.reserve(n_tx);
        HIP_CHECK(hipMemcpyAsync(d_rsrc.p, tx_v, sizeof(T) * 2 * n_tx, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_rt0.p, t0_v, sizeof(T) * n_tx, hipMemcpyHostToDevice, stream));
        RayGeom2<T> rg2;
        rg2.nnx = ncx + 1; rg2.nnz = ncz + 1;
        rg2.dx = dx; rg2.dz = dz; rg2.xmin = xmin; rg2.zmin = zmin; rg2.xmax = xmax; rg2.zmax = zmax;
        const long max_steps = walk_step_limit;
        long cap = walk_room(8L * ((long)ncx + ncz + 3)) + 4;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_rx, ((size_t)256 << 20) / (sizeof(T) * 4 * cap)));
        std::vector<int> st(chunk), np(chunk), nl(chunk);
        std::vector<uint32_t> hc;
        std::vector<T> hv, hp;
        for (int c0 = 0; c0 < n_rx; c0 += chunk) {
            const int m = std::min(chunk, n_rx - c0);
            const T* pc = (const T*)rx_v + 2 * (size_t)c0;
            d_rx.reserve(2 * (size_t)m); d_out.reserve(m); d_rstat.reserve(m); d_raynp.reserve(m); d_lnum.reserve(m);
            HIP_CHECK(hipMemcpyAsync(d_rx.p, pc, sizeof(T) * 2 * m, hipMemcpyHostToDevice, stream));
            for (int attempt = 0;; ++attempt) {
                if (with_rays) d_raypts.reserve((size_t)m * cap * 2);
                d_lcell.reserve((size_t)m * cap); d_lval.reserve((size_t)m * cap);
                const dim3 rgrid((m + 63) / 64), rblock(64);
                if (with_rays)
                    fsm_raypath2d_l<T, true><<<rgrid, rblock, 0, stream>>>(tt_ptr(ps), NS, d_s.p, d_cells.p, rg2, n_tx, d_rsrc.p, d_rt0.p, d_rx.p, m, d_out.p,
                                                                           d_rstat.p, max_steps, d_raypts.p, cap, d_raynp.p, d_lcell.p, d_lval.p, cap, d_lnum.p);
                else
                    fsm_raypath2d_l<T, false><<<rgrid, rblock, 0, stream>>>(tt_ptr(ps), NS, d_s.p, d_cells.p, rg2, n_tx, d_rsrc.p, d_rt0.p, d_rx.p, m, d_out.p,
                                                                            d_rstat.p, max_steps, nullptr, 0, d_raynp.p, d_lcell.p, d_lval.p, cap, d_lnum.p);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(tt_out + c0, d_out.p, sizeof(T) * m, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipMemcpyAsync(st.data(), d_rstat.p, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipMemcpyAsync(nl.data(), d_lnum.p, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
                if (with_rays) HIP_CHECK(hipMemcpyAsync(np.data(), d_raynp.p, sizeof(int) * m, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
                long need = 0;
                for (int q = 0; q < m; ++q) {
                    if (st[q] == 1 || st[q] == 2) throw_walk_error(st[q], pc + 2 * (size_t)q, (const T*)tx_v, max_steps);
                    if (st[q] == 3) need = std::max<long>(need, std::max<long>(nl[q], with_rays ? np[q] : 0) + 1);
                }
                if (need == 0) break;
                if (attempt > 2) throw DeviceError("raypath: a long ray did not retrace to the same length");
                cap = need;   // a ray longer than a row: the chunk once more with the room it asked for
            }
            hc.resize((size_t)m * cap); hv.resize((size_t)m * cap);
            HIP_CHECK(hipMemcpyAsync(hc.data(), d_lcell.p, sizeof(uint32_t) * (size_t)m * cap, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(hv.data(), d_lval.p, sizeof(T) * (size_t)m * cap, hipMemcpyDeviceToHost, stream));
            if (with_rays) { hp.resize((size_t)m * cap * 2); HIP_CHECK(hipMemcpyAsync(hp.data(), d_raypts.p, sizeof(T) * (size_t)m * cap * 2, hipMemcpyDeviceToHost, stream)); }
            HIP_CHECK(hipStreamSynchronize(stream));
            struct Siv { size_t i; T v; };
            std::vector<Siv> row;
            for (int q = 0; q < m; ++q) {
                row.resize(nl[q]);
                for (int e = 0; e < nl[q]; ++e) { row[e].i = hc[(size_t)q * cap + e]; row[e].v = hv[(size_t)q * cap + e]; }
                std::sort(row.begin(), row.end(), [](const Siv n1, const Siv n2) { return n1.i < n2.i; });   // CompareSiv_i
                for (const Siv& e : row) { lcell.push_back((long long)e.i); lval.push_back(e.v); }
                loff.push_back((long long)lcell.size());
                if (with_rays) {
                    rpts.insert(rpts.end(), hp.begin() + (size_t)q * cap * 2, hp.begin() + ((size_t)q * cap + np[q]) * 2);
                    roff.push_back(roff.back() + np[q]);
                }
            }
        }
    }
    void raytrace_l(int slot, int n_tx, const void* tx_v, const void* t0_v, int n_rx, const void* rx_v, void* tt_out_v, bool with_rays) override {
        HIP_CHECK(hipSetDevice(device));
        check_slot(slot);
        if (dim != 2) throw Unsupported("compute_L defined for the FSM");   // (3-D: ttcrpy itself raises, rgrid.pyx:916-917)
        if (!cell) throw Unsupported("compute_L defined only for grids with slowness defined for cells");
        if (n_tx < 1) throw ValueError("every source needs at least one point");
        // the solve (Grid2D::raytrace(Tx, t0, Rx, threadNo)), without receivers: the walk below gives the traveltimes
        {
            const int tx_off[2] = {0, n_tx}, rx_off[2] = {0, 0};
            const int keep_ttrp = ttrp;
            ttrp = 0;
            try { raytrace_multi(1, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, slot); } catch (...) { ttrp = keep_ttrp; throw; }
            ttrp = keep_ttrp;
        }
        if (slot_l_off.empty()) { slot_l_off.assign(n_slots, std::vector<long long>{0}); slot_l_cell.resize(n_slots); slot_l_val.resize(n_slots); }
        if (slot_rays_off.empty()) { slot_rays_off.assign(n_slots, std::vector<long long>{0}); slot_rays_pts.resize(n_slots); }
        walk_l(P(slot), n_tx, tx_v, t0_v, n_rx, rx_v, tt_out_v, with_rays, slot_l_off[slot], slot_l_cell[slot], slot_l_val[slot], slot_rays_off[slot],
               slot_rays_pts[slot]);
    }
    // the l_data overloads for every source of a call (Grid2D's multi-source overloads with l_data run the single-source overload per
    // source on host threads, ttcr/Grid2D.h; ttcrpy: compute_L with several events): batched solves, the walks follow each batch.
    // One CSR over all receiver rows of the call, in row order; the rays (with_rays) as the rays of the call.
    bool l_walk_mode = false, l_walk_rays = false;
    std::vector<std::vector<long long>> l_src_off, l_src_cell, l_src_roff;
    std::vector<std::vector<T>> l_src_val, l_src_rpts;
    std::vector<long long> multi_l_off{0}, multi_l_cell;
    std::vector<T> multi_l_val;
    void raytrace_multi_l(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                          void* tt_out_v, bool with_rays) override {
        if (dim != 2) throw Unsupported("compute_L defined for the FSM");
        if (!cell) throw Unsupported("compute_L defined only for grids with slowness defined for cells");
        multi_l_off.assign(1, 0); multi_l_cell.clear(); multi_l_val.clear();
        rays_off.assign(1, 0); rays_pts.clear();
        if (n_src <= 0) return;
        l_src_off.assign(n_src, {}); l_src_cell.assign(n_src, {}); l_src_roff.assign(n_src, {}); l_src_val.assign(n_src, {}); l_src_rpts.assign(n_src, {});
        const int keep_ttrp = ttrp;
        ttrp = 0;
        l_walk_mode = true; l_walk_rays = with_rays;
        try {
            raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, -1);
        } catch (...) { l_walk_mode = false; ttrp = keep_ttrp; throw; }
        l_walk_mode = false; ttrp = keep_ttrp;
        rays_off.assign(1, 0); rays_pts.clear();
        for (int n = 0; n < n_src; ++n) {
            const long long lbase = (long long)multi_l_cell.size();
            for (size_t r = 1; r < l_src_off[n].size(); ++r) multi_l_off.push_back(lbase + l_src_off[n][r]);
            multi_l_cell.insert(multi_l_cell.end(), l_src_cell[n].begin(), l_src_cell[n].end());
            multi_l_val.insert(multi_l_val.end(), l_src_val[n].begin(), l_src_val[n].end());
            if (with_rays) {
                const long long base = rays_off.back();
                for (size_t r = 1; r < l_src_roff[n].size(); ++r) rays_off.push_back(base + l_src_roff[n][r]);
                rays_pts.insert(rays_pts.end(), l_src_rpts[n].begin(), l_src_rpts[n].end());
            }
        }
    }
    void multi_l_size(size_t* n_rows, size_t* nnz) const override { *n_rows = multi_l_off.size() - 1; *nnz = multi_l_cell.size(); }
    void get_multi_l(long long* row_off, long long* cellv, void* v) const override {
        std::memcpy(row_off, multi_l_off.data(), multi_l_off.size() * sizeof(long long));
        if (!multi_l_cell.empty()) {
            std::memcpy(cellv, multi_l_cell.data(), multi_l_cell.size() * sizeof(long long));
            std::memcpy(v, multi_l_val.data(), multi_l_val.size() * sizeof(T));
        }
    }
    void slot_l_size(int slot, size_t* n_rows, size_t* nnz) const override {
        check_slot(slot);
        if (slot_l_off.empty()) { *n_rows = 0; *nnz = 0; return; }
        *n_rows = slot_l_off[slot].size() - 1;
        *nnz = slot_l_cell[slot].size();
    }
    void get_slot_l(int slot, long long* row_off, long long* cellno, void* v) const override {
        check_slot(slot);
        if (slot_l_off.empty()) { row_off[0] = 0; return; }
        std::memcpy(row_off, slot_l_off[slot].data(), slot_l_off[slot].size() * sizeof(long long));
        if (!slot_l_cell[slot].empty()) {
            std::memcpy(cellno, slot_l_cell[slot].data(), slot_l_cell[slot].size() * sizeof(long long));
            std::memcpy(v, slot_l_val[slot].data(), slot_l_val[slot].size() * sizeof(T));
        }
    }

    // rays of the last raytrace_rays call of every slot
    std::vector<std::vector<long long>> slot_rays_off;
    std::vector<std::vector<T>> slot_rays_pts;
    void raytrace_rays(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out) override {
        check_slot(slot);
        const int tx_off[2] = {0, n_tx}, rx_off[2] = {0, n_rx};
        raytrace_multi(1, tx_off, tx, t0, rx_off, rx, tt_out, slot, nullptr, true);
        if (slot_rays_off.empty()) { slot_rays_off.assign(n_slots, std::vector<long long>{0}); slot_rays_pts.resize(n_slots); }
        slot_rays_off[slot] = rays_off;
        slot_rays_pts[slot].swap(rays_pts);
        if (!return_rays) { rays_off.assign(1, 0); rays_pts.clear(); } else rays_pts = slot_rays_pts[slot];
    }
    void slot_rays_size(int slot, size_t* n_rays, size_t* n_points) const override {
        check_slot(slot);
        if (slot_rays_off.empty()) { *n_rays = 0; *n_points = 0; return; }
        *n_rays = slot_rays_off[slot].size() - 1;
        *n_points = (size_t)slot_rays_off[slot].back();
    }
    void get_slot_rays(int slot, long long* offsets, void* pts) const override {
        check_slot(slot);
        if (slot_rays_off.empty()) { offsets[0] = 0; return; }
        std::memcpy(offsets, slot_rays_off[slot].data(), slot_rays_off[slot].size() * sizeof(long long));
        if (!slot_rays_pts[slot].empty()) std::memcpy(pts, slot_rays_pts[slot].data(), slot_rays_pts[slot].size() * sizeof(T));
    }
    void rays_size(size_t* n_rays, size_t* n_points) const override {
        *n_rays = rays_off.size() - 1;
        *n_points = (size_t)rays_off.back();
    }
    void get_rays(long long* offsets, void* pts) const override {
        std::memcpy(offsets, rays_off.data(), rays_off.size() * sizeof(long long));
        if (!rays_pts.empty()) std::memcpy(pts, rays_pts.data(), rays_pts.size() * sizeof(T));
    }

    // Grid3D::raytrace multi-source overload (ttcr/Grid3D.h:810-853)
    void validate_points(int n_tx, const void* tx_v, int n_rx, const void* rx_v) override {
        const int nc = ncoord();
        if (n_tx <= 0) throw ValueError("every source needs at least one point");
        std::vector<T> tx((const T*)tx_v, (const T*)tx_v + (size_t)nc * n_tx), rx((const T*)rx_v, (const T*)rx_v + (size_t)nc * std::max(n_rx, 0));
        if (translate) {
            for (int m = 0; m < n_tx; ++m) { tx[3 * m] -= ox; tx[3 * m + 1] -= oy; tx[3 * m + 2] -= oz; }
            for (int m = 0; m < n_rx; ++m) { rx[3 * m] -= ox; rx[3 * m + 1] -= oy; rx[3 * m + 2] -= oz; }
        }
        check_pts(tx.data(), n_tx);
        check_pts(rx.data(), n_rx);
    }

    // Source pairs (NS == 2) share the control flow of the sweep kernel: with exact skipping a chunk is evaluated when EITHER
    // source of the pair needs it, so two sources that lie close to each other -- whose fronts reach the same regions in the
    // same sweeps -- cost fewer evaluations than two that do not (64 random sources on 512^3 nodes: 40.5 % -> 33.9 % of the
    // node updates evaluated, 204 -> 175 ms of sweeps).  The results do not depend on who shares a pair with whom.  Within
    // the batch (logical slots sl[b], sources sr[b]) the physical slots are handed out again: greedy nearest-neighbour pairs
    // (first source point) go to the slot pairs the batch owns completely, the rest to its other slots; `phys` records it.
    void pair_sources(const std::vector<int>& sl, const std::vector<int>& sr, const int* tx_off, const T* tx) {
        const int nb = (int)sl.size();
        if (NS != 2 || !pair_by_distance || nb < 3) return;
        const int nc = ncoord();
        std::vector<int> ps(nb);
        for (int b = 0; b < nb; ++b) ps[b] = P(sl[b]);
        std::sort(ps.begin(), ps.end());
        std::vector<int> pair_slots, single_slots;   // physical slots of complete pairs (2g, 2g+1 both in the batch), the others
        for (int b = 0; b < nb;) {
            if (b + 1 < nb && (ps[b] & 1) == 0 && ps[b + 1] == ps[b] + 1) { pair_slots.push_back(ps[b]); pair_slots.push_back(ps[b + 1]); b += 2; }
            else { single_slots.push_back(ps[b]); b += 1; }
        }
        if (pair_slots.empty()) return;
        auto dist2 = [&](int a, int b) {
            double d = 0;
            for (int c = 0; c < nc; ++c) { const double v = (double)tx[(size_t)nc * tx_off[sr[a]] + c] - (double)tx[(size_t)nc * tx_off[sr[b]] + c]; d += v * v; }
            return d;
        };
        std::vector<char> used(nb, 0);
        std::vector<int> order;   // batch entries: pairs first, then what is left
        order.reserve(nb);
        int n_left = nb;
        for (size_t k = 0; k + 1 < pair_slots.size(); k += 2) {
            int a = 0;
            while (used[a]) ++a;
            used[a] = 1;
            int best = -1;
            double bd = 0;
            for (int b = 0; b < nb; ++b)
                if (!used[b]) { const double d = dist2(a, b); if (best < 0 || d < bd) { best = b; bd = d; } }
            used[best] = 1;
            order.push_back(a); order.push_back(best);
            n_left -= 2;
        }
        for (int b = 0; b < nb && n_left > 0; ++b) if (!used[b]) { order.push_back(b); --n_left; }
        std::vector<int> target(pair_slots);
        target.insert(target.end(), single_slots.begin(), single_slots.end());
        for (int k = 0; k < nb; ++k) phys[sl[order[k]]] = target[k];
    }

    void raytrace_multi(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off,
                        const void* rx_v, void* tt_out_v, int forced_slot, const int* explicit_slots = nullptr,
                        bool force_rays = false) override {
        HIP_CHECK(hipSetDevice(device));
        if (host_prof) { hp_t = std::chrono::steady_clock::now(); std::fprintf(stderr, "[host] ---- raytrace_multi\n"); }
        const int return_rays = (this->return_rays.load() || force_rays) ? 1 : 0;   // (shadows the option for this call)
        const auto wall0 = std::chrono::steady_clock::now();
        timing = Timing();
        timing.n_sources = n_src;
        rays_off.assign(1, 0);
        rays_pts.clear();
        if (!have_slowness) throw std::runtime_error("Error: slowness has not been assigned.");
        if (n_src <= 0) return;
        if (forced_slot >= 0) {
            check_slot(forced_slot);
            if (n_src != 1) throw ValueError("a thread number can only be given for a single source");
        }
        const int nc = ncoord();
        const int n_tx = tx_off[n_src], n_rx = rx_off[n_src];
        std::vector<T> tx((const T*)tx_v, (const T*)tx_v + (size_t)nc * n_tx);
        std::vector<T> rx((const T*)rx_v, (const T*)rx_v + (size_t)nc * n_rx);
        const T* t0 = (const T*)t0_v;
        T* tt_out = (T*)tt_out_v;
        if (translate) {  // Grid3D::raytrace subtracts the origin (ttcr/Grid3D.h:478-485)
            for (int m = 0; m < n_tx; ++m) { tx[3 * m] -= ox; tx[3 * m + 1] -= oy; tx[3 * m + 2] -= oz; }
            for (int m = 0; m < n_rx; ++m) { rx[3 * m] -= ox; rx[3 * m + 1] -= oy; rx[3 * m + 2] -= oz; }
        }
        for (int n = 0; n < n_src; ++n) {
            if (tx_off[n + 1] <= tx_off[n]) throw ValueError("every source needs at least one point");
            check_pts(tx.data() + (size_t)nc * tx_off[n], tx_off[n + 1] - tx_off[n]);
            check_pts(rx.data() + (size_t)nc * rx_off[n], rx_off[n + 1] - rx_off[n]);
        }
        if (explicit_slots)
            for (int n = 0; n < n_src; ++n) {
                check_slot(explicit_slots[n]);
                if (n > 0 && explicit_slots[n] <= explicit_slots[n - 1]) throw ValueError("explicit slots must be ascending and distinct");
            }
        // block distribution of the sources over the slots: get_blk_size (ttcr/Grid3D.h:451-465)
        const int n_blk = explicit_slots ? n_src : std::min(n_slots, n_src);
        std::vector<int> blk(n_blk, 0);
        for (int n = 0; n < n_src; ++n) blk[n % n_blk] += 1;
        std::vector<int> start(n_blk, 0);
        for (int b = 1; b < n_blk; ++b) start[b] = start[b - 1] + blk[b - 1];
        const int rounds = *std::max_element(blk.begin(), blk.end());
        const int mb = std::max(1, std::min(max_batch > 0 ? max_batch : n_slots, n_slots));
        std::vector<std::vector<long long>> src_ray_len(return_rays ? n_src : 0);
        std::vector<std::vector<T>> src_ray_pts(return_rays ? n_src : 0);
        for (int r = 0; r < rounds; ++r) {
            std::vector<int> slots, srcs;
            for (int b = 0; b < n_blk; ++b)
                if (r < blk[b]) { slots.push_back(forced_slot >= 0 ? forced_slot : (explicit_slots ? explicit_slots[b] : b)); srcs.push_back(start[b] + r); }
            for (size_t c0 = 0; c0 < slots.size(); c0 += mb) {
                const size_t c1 = std::min(slots.size(), c0 + mb);
                std::vector<int> sl(slots.begin() + c0, slots.begin() + c1), sr(srcs.begin() + c0, srcs.begin() + c1);
                // logical -> physical slots; the sources of a block-distributed batch are first paired by distance
                // (also when the caller names the slots -- the replicas of a multi-device grid, single-source calls of several host
                // threads that went to the device together: the permutation stays among the slots of the batch)
                if ((int)sl.size() == n_slots) choose_layout();   // (every slot restarts: the layout may follow the model, see the constructor)
                if (forced_slot < 0) pair_sources(sl, sr, tx_off, tx.data());
                for (int& q : sl) q = P(q);
                {   // (the batch driver takes its entries in ascending slot order)
                    std::vector<int> idx(sl.size());
                    for (size_t q = 0; q < idx.size(); ++q) idx[q] = (int)q;
                    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return sl[a] < sl[b]; });
                    std::vector<int> sl2(sl.size()), sr2(sr.size());
                    for (size_t q = 0; q < idx.size(); ++q) { sl2[q] = sl[idx[q]]; sr2[q] = sr[idx[q]]; }
                    sl.swap(sl2); sr.swap(sr2);
                }
                solve_batch(sl, sr, tx_off, tx.data(), t0);
                hp_mark("solve_batch tail");
                if (adj_sink) {
                    // the field tape: interpolated receiver traveltimes whatever tt_from_rp says, then the batch's fields and lists
                    interp_batch(sl, sr, rx_off, rx.data(), tt_out);
                    adj_record(sl, sr, tx_off, tx.data(), t0, rx_off, rx.data());
                } else if (l_walk_mode) {
                    // the l_data overloads for every source of the call (raytrace_multi_l): the walk gives traveltimes, entries and rays
                    for (size_t b = 0; b < sl.size(); ++b) {
                        const int n = sr[b];
                        walk_l(sl[b], tx_off[n + 1] - tx_off[n], tx.data() + (size_t)2 * tx_off[n], t0 + tx_off[n], rx_off[n + 1] - rx_off[n],
                               rx.data() + (size_t)2 * rx_off[n], tt_out + rx_off[n], l_walk_rays, l_src_off[n], l_src_cell[n], l_src_val[n],
                               l_src_roff[n], l_src_rpts[n]);
                    }
                } else if (m_walk_mode) {
                    // the m_data overloads for every source of the call (raytrace_multi_m): the rays of the overload that keeps them,
                    // then the walk that leaves the terms of M -- its traveltimes are the call's
                    if (return_rays) raypath_batch_rays(sl, sr, tx_off, tx.data(), t0, rx_off, rx.data(), tt_out, src_ray_len, src_ray_pts);
                    for (size_t b = 0; b < sl.size(); ++b) {
                        const int n = sr[b];
                        walk_m(sl[b], tx_off[n + 1] - tx_off[n], tx.data() + (size_t)3 * tx_off[n], t0 + tx_off[n], rx_off[n + 1] - rx_off[n],
                               rx.data() + (size_t)3 * rx_off[n], tt_out + rx_off[n], m_walk_both, m_seg_off[n], m_segs[n],
                               m_tape_src.empty() ? nullptr : &m_tape_src[n], rx_off[n]);
                    }
                } else if (!(ttrp || return_rays)) {
                    interp_batch(sl, sr, rx_off, rx.data(), tt_out);
                    hp_mark("receivers");
                } else if (!return_rays) {
                    raypath_batch(sl, sr, tx_off, tx.data(), t0, rx_off, rx.data(), tt_out);
                } else {
                    raypath_batch_rays(sl, sr, tx_off, tx.data(), t0, rx_off, rx.data(), tt_out, src_ray_len, src_ray_pts);
                }
            }
        }
        if (return_rays) {   // one ray per receiver row, in row order (rows of source 0, then source 1, ...)
            size_t tot = 0;
            for (int n = 0; n < n_src; ++n) tot += src_ray_pts[n].size();
            rays_pts.reserve(tot);
            for (int n = 0; n < n_src; ++n) {
                for (long long len : src_ray_len[n]) rays_off.push_back(rays_off.back() + len);
                rays_pts.insert(rays_pts.end(), src_ray_pts[n].begin(), src_ray_pts[n].end());
                std::vector<T>().swap(src_ray_pts[n]);
            }
        }
        timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
};

// ---- one grid on several devices ---------------------------------------------------------------------------
// Replaces, for more than one GPU, what Grid3D's multi-source overload does with host threads (ttcr/Grid3D.h:810-853;
// the reference's OpenCL backend keeps one solver per thread slot in one process, ttcr/Grid3Drnfs_OpenCL.h:172-193):
// one replica of the grid per device (slowness replicated, traveltime slots divided), the sources of a call block-
// distributed over the slots exactly like get_blk_size (ttcr/Grid3D.h:451-465), slot s living on device s / spd
// (spd = slots per device), one host thread per device driving its replica, no exchange between devices during a
// solve.  Everything else (getTT, receivers, iteration counts, rays) is forwarded to the replica that owns the slot.
class MultiGrid : public GridBase {
   public:
    std::vector<std::unique_ptr<GridBase>> rep;
    int spd = 1;   // slots per replica (the last one may hold fewer)
    std::vector<long long> rays_off{0};
    std::vector<char> rays_pts;
    size_t pt_bytes = 12;

    template <typename Make>
    MultiGrid(int n_slots_, const std::vector<int>& devs, Make&& make) {
        n_slots = n_slots_;
        const int nd = std::min<int>((int)devs.size(), n_slots);
        spd = (n_slots + nd - 1) / nd;
        for (int r = 0; r * spd < n_slots; ++r) rep.emplace_back(make(std::min(spd, n_slots - r * spd), devs[r]));
        const GridBase& g0 = *rep[0];
        dim = g0.dim; dtype = g0.dtype; device = g0.device; n_nodes = g0.n_nodes; n_cells = g0.n_cells;
        elem_size = g0.elem_size; weno = g0.weno;
        pt_bytes = elem_size * (dim == 3 ? 3 : 2);
        niter.assign(n_slots, 0);
        niterw.assign(n_slots, 0);
        // the slowness of one device is handed to the others device to device
        for (size_t a = 0; a < rep.size(); ++a)
            for (size_t b = 0; b < rep.size(); ++b)
                if (rep[a]->device != rep[b]->device) {
                    (void)hipSetDevice(rep[a]->device);
                    (void)hipDeviceEnablePeerAccess(rep[b]->device, 0);   // (already enabled / not possible: the copy is staged)
                    (void)hipGetLastError();
                }
    }
    GridBase& of(int slot, int& local) const {
        if (slot < 0 || slot >= n_slots) throw ValueError("Thread number is larger than number of threads");
        local = slot % spd;
        return *rep[slot / spd];
    }
    void apply_option(const std::string& k, double value) override {
        GridBase::apply_option(k, value);
        for (auto& r : rep) r->apply_option(k, value);
    }
    void set_slowness(const void* s, size_t n, bool on_device, bool c_order = false) override {
        for (auto& r : rep) r->set_slowness(s, n, on_device, c_order);
    }
    void get_slowness(void* out, size_t n) override { rep[0]->get_slowness(out, n); }
    void validate_points(int n_tx, const void* tx, int n_rx, const void* rx) override { rep[0]->validate_points(n_tx, tx, n_rx, rx); }
    void get_tt(int slot, void* out, size_t n) override { int l; GridBase& g = of(slot, l); g.get_tt(l, out, n); }
    void* tt_device(int slot) override { int l; GridBase& g = of(slot, l); return g.tt_device(l); }
    void* tt_device_view(int slot, size_t* stride) override { int l; GridBase& g = of(slot, l); return g.tt_device_view(l, stride); }
    void interp(int slot, int n, const void* pts, void* out) override { int l; GridBase& g = of(slot, l); g.interp(l, n, pts, out); }
    void compute_slowness(int n, const void* pts, bool translated, void* out) override { rep[0]->compute_slowness(n, pts, translated, out); }
    void get_niter(int slot, int* it, int* itw) const override { int l; GridBase& g = of(slot, l); g.get_niter(l, it, itw); }
    std::string kernel_name() const override { return rep[0]->kernel_name(); }
    long long prefill_swap_count() const override { long long a = 0; for (const auto& r : rep) a += r->prefill_swap_count(); return a; }
    long long prefill_inline_count() const override { long long a = 0; for (const auto& r : rep) a += r->prefill_inline_count(); return a; }
    void stopping_stats(long long* sums, long long* missed, long long* rounds) const override {
        long long a = 0, b = 0, c = 0;
        for (const auto& r : rep) { long long x = 0, y = 0, z = 0; r->stopping_stats(&x, &y, &z); a += x; b += y; c += z; }
        if (sums) *sums = a;
        if (missed) *missed = b;
        if (rounds) *rounds = c;
    }
    void reference_change_host(const void* times, const void* field, bool parallel, void* out) override { rep[0]->reference_change_host(times, field, parallel, out); }
    void get_changes(int slot, double* first, int n_first, double* wen, int n_weno) const override {
        int l; GridBase& g = of(slot, l); g.get_changes(l, first, n_first, wen, n_weno);
    }
    void get_reference_changes(int slot, double* first, int n_first, double* wen, int n_weno) const override {
        int l; GridBase& g = of(slot, l); g.get_reference_changes(l, first, n_first, wen, n_weno);
    }
    void rays_size(size_t* n_rays, size_t* n_points) const override { *n_rays = rays_off.size() - 1; *n_points = (size_t)rays_off.back(); }
    void get_rays(long long* offsets, void* pts) const override {
        std::memcpy(offsets, rays_off.data(), rays_off.size() * sizeof(long long));
        if (!rays_pts.empty()) std::memcpy(pts, rays_pts.data(), rays_pts.size());
    }
    void raytrace_rays(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out) override {
        int l; GridBase& g = of(slot, l);
        g.raytrace_rays(l, n_tx, tx, t0, n_rx, rx, tt_out);
        timing = g.timing;
    }
    void raytrace_m(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out, bool both) override {
        int l; GridBase& g = of(slot, l);
        g.raytrace_m(l, n_tx, tx, t0, n_rx, rx, tt_out, both);
        timing = g.timing;
    }
    void slot_m_size(int slot, size_t* n_rows, size_t* nnz) const override { int l; GridBase& g = of(slot, l); g.slot_m_size(l, n_rows, nnz); }
    // The batched m_data / l_data calls (Grid3D::raytrace with m_data, Grid2D::raytrace with l_data, for every event of a call): the
    // sources go to the replicas in contiguous blocks, in proportion to their slots (every replica then distributes its block over
    // its own slots like a one-device grid), the replicas work side by side, and the CSR rows, rays and traveltimes of the blocks are
    // put together in source order.
    std::vector<long long> mm_off{0}, mm_idx;
    std::vector<char> mm_val;
    template <typename Call, typename Size, typename Get>
    void sharded_matrix_call(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v, void* tt_out_v,
                             Call&& call, Size&& size_of, Get&& get_of) {
        const auto wall0 = std::chrono::steady_clock::now();
        timing = Timing();
        timing.n_sources = n_src;
        mm_off.assign(1, 0); mm_idx.clear(); mm_val.clear();
        rays_off.assign(1, 0); rays_pts.clear();
        if (n_src <= 0) return;
        const char* tx = (const char*)tx_v; const char* t0 = (const char*)t0_v; const char* rx = (const char*)rx_v;
        char* tt_out = (char*)tt_out_v;
        const int nd = (int)rep.size();
        std::vector<int> first(nd + 1, 0);   // sources [first[d], first[d+1]) go to replica d
        {
            long long before = 0;
            for (int d = 0; d < nd; ++d) {
                first[d] = (int)((long long)n_src * before / n_slots);
                before += rep[d]->n_slots;
            }
            first[nd] = n_src;
        }
        struct Part { std::vector<long long> off, idx, roff; std::vector<char> val, rpts; Timing t; };
        std::vector<Part> part(nd);
        std::vector<std::exception_ptr> errs(nd);
        auto work = [&](int d) {
            try {
                const int s0 = first[d], m = first[d + 1] - first[d];
                if (m <= 0) return;
                GridBase& g = *rep[d];
                std::vector<int> to(m + 1), ro(m + 1);
                for (int q = 0; q <= m; ++q) { to[q] = tx_off[s0 + q] - tx_off[s0]; ro[q] = rx_off[s0 + q] - rx_off[s0]; }
                std::vector<char> stt(elem_size * (size_t)std::max(ro[m], 1));
                call(g, m, to.data(), tx + pt_bytes * tx_off[s0], t0 + elem_size * tx_off[s0], ro.data(), rx + pt_bytes * rx_off[s0], stt.data());
                std::memcpy(tt_out + elem_size * rx_off[s0], stt.data(), elem_size * (size_t)ro[m]);
                Part& p = part[d];
                p.t = g.timing;
                size_t nr = 0, nnz = 0;
                size_of(g, &nr, &nnz);
                p.off.assign(nr + 1, 0); p.idx.resize(nnz); p.val.resize(nnz * elem_size);
                if (nr > 0) get_of(g, p.off.data(), p.idx.data(), p.val.data());
                size_t rr = 0, rp = 0;
                g.rays_size(&rr, &rp);
                p.roff.assign(rr + 1, 0); p.rpts.resize(rp * pt_bytes);
                if (rr > 0) g.get_rays(p.roff.data(), p.rpts.data());
            } catch (...) { errs[d] = std::current_exception(); }
        };
        std::vector<std::thread> th;
        for (int d = 1; d < nd; ++d) th.emplace_back(work, d);
        work(0);
        for (auto& t : th) t.join();
        for (auto& e : errs)
            if (e) std::rethrow_exception(e);
        for (int d = 0; d < nd; ++d) {
            const Part& p = part[d];
            if (p.off.empty()) continue;
            const long long base = mm_off.back();
            for (size_t r = 1; r < p.off.size(); ++r) mm_off.push_back(base + p.off[r]);
            mm_idx.insert(mm_idx.end(), p.idx.begin(), p.idx.end());
            mm_val.insert(mm_val.end(), p.val.begin(), p.val.end());
            const long long rbase = rays_off.back();
            for (size_t r = 1; r < p.roff.size(); ++r) rays_off.push_back(rbase + p.roff[r]);
            rays_pts.insert(rays_pts.end(), p.rpts.begin(), p.rpts.end());
            timing.sweep_ms = std::max(timing.sweep_ms, p.t.sweep_ms);   // (the devices run side by side)
            timing.launches += p.t.launches;
            timing.node_updates += p.t.node_updates;
            timing.evaluated_updates += p.t.evaluated_updates;
            timing.iterations = std::max(timing.iterations, p.t.iterations);
        }
        // iteration counts: per slot, as after any call (the last source a slot solved)
        for (int s2 = 0; s2 < n_slots; ++s2) { int l; GridBase& g = of(s2, l); g.get_niter(l, &niter[s2], &niterw[s2]); }
        timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    void raytrace_multi_m(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx, void* tt_out,
                          bool both) override {
        sharded_matrix_call(
            n_src, tx_off, tx, t0, rx_off, rx, tt_out,
            [&](GridBase& g, int m, const int* to, const void* stx, const void* st0, const int* ro, const void* srx, void* stt) {
                g.raytrace_multi_m(m, to, stx, st0, ro, srx, stt, both);
            },
            [](GridBase& g, size_t* nr, size_t* nnz) { g.multi_m_size(nr, nnz); },
            [](GridBase& g, long long* off, long long* idx, void* v) { g.get_multi_m(off, idx, v); });
    }
    // The M tape: the sources go to the replicas like sharded_matrix_call sends them, every replica merges its rows on its own device, and
    // the parts are put together in row order on the first device (rows shifted by the receiver rows in front of the part).
    void raytrace_multi_tape(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                             void* tt_out_v, TapeRows& out) override {
        if (dim != 3) throw Unsupported("compute_M is implemented for 3-D grids only");
        const auto wall0 = std::chrono::steady_clock::now();
        timing = Timing();
        timing.n_sources = n_src;
        HIP_CHECK(hipSetDevice(rep[0]->device));
        out.release();
        out.elem = elem_size;
        if (n_src <= 0) return;
        const char* tx = (const char*)tx_v; const char* t0 = (const char*)t0_v; const char* rx = (const char*)rx_v;
        char* tt_out = (char*)tt_out_v;
        const int nd = (int)rep.size();
        std::vector<int> first(nd + 1, 0);
        {
            long long before = 0;
            for (int d = 0; d < nd; ++d) {
                first[d] = (int)((long long)n_src * before / n_slots);
                before += rep[d]->n_slots;
            }
            first[nd] = n_src;
        }
        std::vector<TapeRows> part(nd);
        std::vector<Timing> pt(nd);
        std::vector<std::exception_ptr> errs(nd);
        auto work = [&](int d) {
            try {
                const int s0 = first[d], m = first[d + 1] - first[d];
                if (m <= 0) return;
                GridBase& g = *rep[d];
                std::vector<int> to(m + 1), ro(m + 1);
                for (int q = 0; q <= m; ++q) { to[q] = tx_off[s0 + q] - tx_off[s0]; ro[q] = rx_off[s0 + q] - rx_off[s0]; }
                std::vector<char> stt(elem_size * (size_t)std::max(ro[m], 1));
                g.raytrace_multi_tape(m, to.data(), tx + pt_bytes * tx_off[s0], t0 + elem_size * tx_off[s0], ro.data(), rx + pt_bytes * rx_off[s0],
                                      stt.data(), part[d]);
                std::memcpy(tt_out + elem_size * rx_off[s0], stt.data(), elem_size * (size_t)ro[m]);
                pt[d] = g.timing;
            } catch (...) { errs[d] = std::current_exception(); }
        };
        std::vector<std::thread> th;
        for (int d = 1; d < nd; ++d) th.emplace_back(work, d);
        work(0);
        for (auto& t : th) t.join();
        auto drop_parts = [&] {
            for (int d = 0; d < nd; ++d) { (void)hipSetDevice(rep[d]->device); part[d].release(); }
            (void)hipSetDevice(rep[0]->device);
        };
        for (auto& e : errs)
            if (e) { drop_parts(); std::rethrow_exception(e); }
        HIP_CHECK(hipSetDevice(rep[0]->device));
        size_t tot = 0;
        for (const TapeRows& r : part) tot += r.n;
        try {
            out.grow(tot, nullptr);
            for (int d = 0; d < nd; ++d) {
                const TapeRows& r = part[d];
                if (r.n == 0) continue;
                // (device to device across replicas: peer access where the constructor could enable it, staged otherwise)
                HIP_CHECK(hipMemcpy(out.row + out.n, r.row, r.n * sizeof(int), hipMemcpyDefault));
                HIP_CHECK(hipMemcpy(out.col + out.n, r.col, r.n * sizeof(int), hipMemcpyDefault));
                HIP_CHECK(hipMemcpy((char*)out.val + out.n * elem_size, r.val, r.n * elem_size, hipMemcpyDefault));
                tape_shift_rows(out.row + out.n, r.n, rx_off[first[d]], nullptr);
                out.n += r.n;
            }
            HIP_CHECK(hipDeviceSynchronize());
        } catch (...) { drop_parts(); throw; }
        drop_parts();
        for (int d = 0; d < nd; ++d) {
            timing.sweep_ms = std::max(timing.sweep_ms, pt[d].sweep_ms);
            timing.launches += pt[d].launches;
            timing.node_updates += pt[d].node_updates;
            timing.evaluated_updates += pt[d].evaluated_updates;
            timing.iterations = std::max(timing.iterations, pt[d].iterations);
        }
        for (int s2 = 0; s2 < n_slots; ++s2) { int l; GridBase& g = of(s2, l); g.get_niter(l, &niter[s2], &niterw[s2]); }
        timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    // The field tape: the sources go to the replicas like raytrace_multi sends them; every replica copies its fields to the sink's device.
    void adjoint_geometry(int* nn3, double* spacing, TapeWrt wrt) const override { rep[0]->adjoint_geometry(nn3, spacing, wrt); }
    void raytrace_multi_adjoint(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                                void* tt_out_v, AdjSink& sink) override {
        int nn3[3];
        double sp;
        adjoint_geometry(nn3, &sp, sink.cells ? WRT_CELLS : WRT_NODES);
        for (auto& r : rep) r->adj_sink = &sink;
        auto clear = [&] { for (auto& r : rep) { r->adj_sink = nullptr; r->adj_src.clear(); r->adj_row.clear(); } };
        try {
            raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, -1, nullptr, false);
        } catch (...) { clear(); throw; }
        clear();
    }
    void raytrace_multi_l(int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off, const void* rx, void* tt_out,
                          bool with_rays) override {
        sharded_matrix_call(
            n_src, tx_off, tx, t0, rx_off, rx, tt_out,
            [&](GridBase& g, int m, const int* to, const void* stx, const void* st0, const int* ro, const void* srx, void* stt) {
                g.raytrace_multi_l(m, to, stx, st0, ro, srx, stt, with_rays);
            },
            [](GridBase& g, size_t* nr, size_t* nnz) { g.multi_l_size(nr, nnz); },
            [](GridBase& g, long long* off, long long* idx, void* v) { g.get_multi_l(off, idx, v); });
    }
    void multi_l_size(size_t* n_rows, size_t* nnz) const override { *n_rows = mm_off.size() - 1; *nnz = mm_idx.size(); }
    void get_multi_l(long long* row_off, long long* cell, void* v) const override { get_multi_m(row_off, cell, v); }
    void multi_m_size(size_t* n_rows, size_t* nnz) const override { *n_rows = mm_off.size() - 1; *nnz = mm_idx.size(); }
    void get_multi_m(long long* row_off, long long* j, void* v) const override {
        std::memcpy(row_off, mm_off.data(), mm_off.size() * sizeof(long long));
        if (!mm_idx.empty()) {
            std::memcpy(j, mm_idx.data(), mm_idx.size() * sizeof(long long));
            std::memcpy(v, mm_val.data(), mm_val.size());
        }
    }
    void raytrace_l(int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx, void* tt_out, bool with_rays) override {
        int l; GridBase& g = of(slot, l);
        g.raytrace_l(l, n_tx, tx, t0, n_rx, rx, tt_out, with_rays);
        timing = g.timing;
    }
    void slot_l_size(int slot, size_t* n_rows, size_t* nnz) const override { int l; GridBase& g = of(slot, l); g.slot_l_size(l, n_rows, nnz); }
    void get_slot_l(int slot, long long* row_off, long long* cellno, void* v) const override { int l; GridBase& g = of(slot, l); g.get_slot_l(l, row_off, cellno, v); }
    void get_slot_m(int slot, long long* row_off, long long* j, void* v) const override { int l; GridBase& g = of(slot, l); g.get_slot_m(l, row_off, j, v); }
    void slot_rays_size(int slot, size_t* n_rays, size_t* n_points) const override { int l; GridBase& g = of(slot, l); g.slot_rays_size(l, n_rays, n_points); }
    void get_slot_rays(int slot, long long* offsets, void* pts) const override { int l; GridBase& g = of(slot, l); g.get_slot_rays(l, offsets, pts); }

    void raytrace_multi(int n_src, const int* tx_off, const void* tx_v, const void* t0_v, const int* rx_off, const void* rx_v,
                        void* tt_out_v, int forced_slot, const int* explicit_slots = nullptr, bool force_rays = false) override {
        const auto wall0 = std::chrono::steady_clock::now();
        timing = Timing();
        timing.n_sources = n_src;
        rays_off.assign(1, 0);
        rays_pts.clear();
        if (n_src <= 0) return;
        const bool want_rays = return_rays.load() || force_rays;
        const char* tx = (const char*)tx_v; const char* t0 = (const char*)t0_v; const char* rx = (const char*)rx_v;
        char* tt_out = (char*)tt_out_v;
        if (forced_slot >= 0) {
            if (n_src != 1) throw ValueError("a thread number can only be given for a single source");
            int l; GridBase& g = of(forced_slot, l);
            g.raytrace_multi(n_src, tx_off, tx_v, t0_v, rx_off, rx_v, tt_out_v, l, nullptr, force_rays);
            timing = g.timing;
            if (want_rays) {
                size_t nr = 0, np = 0;
                g.rays_size(&nr, &np);
                rays_off.resize(nr + 1);
                rays_pts.resize(np * pt_bytes);
                g.get_rays(rays_off.data(), rays_pts.data());
            }
            return;
        }
        // every point of the call is checked before anything is solved, like on one device
        for (int n = 0; n < n_src; ++n) {
            if (tx_off[n + 1] <= tx_off[n]) throw ValueError("every source needs at least one point");
            rep[0]->validate_points(tx_off[n + 1] - tx_off[n], tx + pt_bytes * tx_off[n], rx_off[n + 1] - rx_off[n], rx + pt_bytes * rx_off[n]);
        }
        // (source, slot, round): the block distribution of get_blk_size over ALL slots, or the slots the caller names
        struct Item { int src, slot, round; };
        std::vector<Item> items;
        if (explicit_slots) {
            for (int n = 0; n < n_src; ++n) {
                if (explicit_slots[n] < 0 || explicit_slots[n] >= n_slots) throw ValueError("Thread number is larger than number of threads");
                if (n > 0 && explicit_slots[n] <= explicit_slots[n - 1]) throw ValueError("explicit slots must be ascending and distinct");
                items.push_back({n, explicit_slots[n], 0});
            }
        } else {
            const int n_blk = std::min(n_slots, n_src);
            std::vector<int> blk(n_blk, 0), start(n_blk, 0);
            for (int n = 0; n < n_src; ++n) blk[n % n_blk] += 1;
            for (int b = 1; b < n_blk; ++b) start[b] = start[b - 1] + blk[b - 1];
            for (int b = 0; b < n_blk; ++b)
                for (int r = 0; r < blk[b]; ++r) items.push_back({start[b] + r, b, r});
        }
        int rounds = 0;
        for (const Item& it : items) rounds = std::max(rounds, it.round + 1);
        std::vector<std::vector<long long>> src_ray_len(want_rays ? n_src : 0);
        std::vector<std::vector<char>> src_ray_pts(want_rays ? n_src : 0);
        std::vector<std::exception_ptr> errs(rep.size());
        std::vector<Timing> dev_t(rep.size());
        auto work = [&](int d) {
            try {
                GridBase& g = *rep[d];
                for (int r = 0; r < rounds; ++r) {
                    std::vector<Item> mine;
                    for (const Item& it : items)
                        if (it.round == r && it.slot / spd == d) mine.push_back(it);
                    if (mine.empty()) continue;
                    std::sort(mine.begin(), mine.end(), [](const Item& a, const Item& b) { return a.slot < b.slot; });
                    const int m = (int)mine.size();
                    std::vector<int> to(m + 1, 0), ro(m + 1, 0), ls(m);
                    for (int q = 0; q < m; ++q) {
                        to[q + 1] = to[q] + tx_off[mine[q].src + 1] - tx_off[mine[q].src];
                        ro[q + 1] = ro[q] + rx_off[mine[q].src + 1] - rx_off[mine[q].src];
                        ls[q] = mine[q].slot % spd;
                    }
                    std::vector<char> stx(pt_bytes * to[m]), st0(elem_size * to[m]), srx(pt_bytes * std::max(ro[m], 1)), stt(elem_size * std::max(ro[m], 1));
                    for (int q = 0; q < m; ++q) {
                        const int n = mine[q].src;
                        std::memcpy(stx.data() + pt_bytes * to[q], tx + pt_bytes * tx_off[n], pt_bytes * (to[q + 1] - to[q]));
                        std::memcpy(st0.data() + elem_size * to[q], t0 + elem_size * tx_off[n], elem_size * (to[q + 1] - to[q]));
                        std::memcpy(srx.data() + pt_bytes * ro[q], rx + pt_bytes * rx_off[n], pt_bytes * (ro[q + 1] - ro[q]));
                    }
                    if (g.adj_sink) {
                        g.adj_src.resize(m);
                        g.adj_row.resize(m);
                        for (int q = 0; q < m; ++q) { g.adj_src[q] = mine[q].src; g.adj_row[q] = rx_off[mine[q].src]; }
                    }
                    g.raytrace_multi(m, to.data(), stx.data(), st0.data(), ro.data(), srx.data(), stt.data(), -1, ls.data(), want_rays);
                    dev_t[d].sweep_ms += g.timing.sweep_ms;
                    dev_t[d].launches += g.timing.launches;
                    dev_t[d].node_updates += g.timing.node_updates;
                    dev_t[d].evaluated_updates += g.timing.evaluated_updates;
                    dev_t[d].iterations = std::max(dev_t[d].iterations, g.timing.iterations);
                    for (int q = 0; q < m; ++q)
                        std::memcpy(tt_out + elem_size * rx_off[mine[q].src], stt.data() + elem_size * ro[q], elem_size * (ro[q + 1] - ro[q]));
                    if (want_rays) {   // the replica's rays are in the row order of ITS call
                        size_t nr = 0, np = 0;
                        g.rays_size(&nr, &np);
                        std::vector<long long> off(nr + 1);
                        std::vector<char> pts(np * pt_bytes);
                        g.get_rays(off.data(), pts.data());
                        for (int q = 0; q < m; ++q) {
                            const int n = mine[q].src;
                            for (int k = ro[q]; k < ro[q + 1]; ++k) src_ray_len[n].push_back(off[k + 1] - off[k]);
                            src_ray_pts[n].assign(pts.begin() + off[ro[q]] * pt_bytes, pts.begin() + off[ro[q + 1]] * pt_bytes);
                        }
                    }
                }
            } catch (...) { errs[d] = std::current_exception(); }
        };
        std::vector<std::thread> th;
        for (size_t d = 1; d < rep.size(); ++d) th.emplace_back(work, (int)d);
        work(0);
        for (auto& t : th) t.join();
        for (auto& e : errs)
            if (e) std::rethrow_exception(e);
        for (int s2 = 0; s2 < n_slots; ++s2) { int l; GridBase& g = of(s2, l); g.get_niter(l, &niter[s2], &niterw[s2]); }
        for (const Timing& t : dev_t) {   // the devices run side by side: times are the slowest one's, counts add up
            timing.sweep_ms = std::max(timing.sweep_ms, t.sweep_ms);
            timing.launches += t.launches;
            timing.node_updates += t.node_updates;
            timing.evaluated_updates += t.evaluated_updates;
            timing.iterations = std::max(timing.iterations, t.iterations);
        }
        if (want_rays)
            for (int n = 0; n < n_src; ++n) {
                for (long long len : src_ray_len[n]) rays_off.push_back(rays_off.back() + len);
                rays_pts.insert(rays_pts.end(), src_ray_pts[n].begin(), src_ray_pts[n].end());
            }
        timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
};

}  // namespace ttcr_amd

// =============================================================================== C ABI
using namespace ttcr_amd;

struct ttcr_fsm_grid {
    std::unique_ptr<GridBase> impl;
};

template <typename F>
static int guarded(F&& f) {
    try {
        f();
        return TTCR_OK;
    } catch (const ValueError& e) {
        g_last_error = e.what();
        return TTCR_ERR_VALUE;
    } catch (const DeviceError& e) {
        g_last_error = e.what();
        return TTCR_ERR_DEVICE;
    } catch (const Unsupported& e) {
        g_last_error = e.what();
        return TTCR_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return TTCR_ERR_RUNTIME;
    }
}

// entry points that touch a grid: serialised per handle (ttcrpy's raytrace(..., thread_no=k) lets several host
// threads work on one grid; here the slots share one stream, one graph and the pinned / scratch buffers)
template <typename G, typename F>
static int guarded_on(G* g, F&& f) {
    if (!g) {
        g_last_error = "null grid handle";
        return TTCR_ERR_VALUE;
    }
    std::lock_guard<std::mutex> lock(g->impl->mu);
    return guarded(std::forward<F>(f));
}

// (the field tape's kernel unit reports device failures with its own exception type)
template <typename F>
static void adj_device_errors(F&& f) {
    try {
        f();
    } catch (const ttcr_amd::AdjDeviceError& e) { throw DeviceError(e.what()); }
}

static int pick_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        throw DeviceError("no HIP device available: the MI355X FSM backend has no CPU fallback");
    if (device < 0) {
        int cur = 0;
        HIP_CHECK(hipGetDevice(&cur));
        return cur;
    }
    if (device >= n) throw ValueError("device ordinal out of range");
    return device;
}

// device list of a grid: the caller's, else TTCR_AMD_DEVICES ("0,1,2,3") when the caller asks for "the current device"
// (an unmodified ttcrpy script is spread over the GPUs of a node by setting the variable), else the one device
static std::vector<int> device_list(int device, const int* devices, int n_devices) {
    std::vector<int> devs;
    if (devices && n_devices > 0) {
        for (int q = 0; q < n_devices; ++q) devs.push_back(pick_device(devices[q]));
    } else if (device < 0 && std::getenv("TTCR_AMD_DEVICES") && *std::getenv("TTCR_AMD_DEVICES")) {
        std::stringstream ss(std::getenv("TTCR_AMD_DEVICES"));
        std::string tok;
        while (std::getline(ss, tok, ',')) {
            if (tok.empty()) continue;
            char* endp = nullptr;
            const long v = std::strtol(tok.c_str(), &endp, 10);
            if (*endp) throw ValueError("TTCR_AMD_DEVICES: expected a comma-separated list of device ordinals");
            devs.push_back(pick_device((int)v));
        }
    }
    if (devs.empty()) devs.push_back(pick_device(device));
    return devs;
}

template <typename Make>
static std::unique_ptr<GridBase> make_grid(int n_slots, const std::vector<int>& devs, Make&& make) {
    if (devs.size() == 1 || n_slots == 1) return std::unique_ptr<GridBase>(make(n_slots, devs[0]));
    return std::unique_ptr<GridBase>(new MultiGrid(n_slots, devs, make));
}

static void create3d(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy, uint32_t ncz, double dx,
                     double xmin, double ymin, double zmin, double eps, int maxit, int weno, int translate_origin, int n_slots,
                     int device, const int* devices, int n_devices) {
    if (!out) throw ValueError("null output handle");
    *out = nullptr;
    if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
    if (ncx < 1 || ncy < 1 || ncz < 1) throw ValueError("grid needs at least one cell per axis");
    if (n_slots < 1) throw ValueError("n_slots must be >= 1");
    if (!(dx > 0)) throw ValueError("dx must be positive");
    if (weno && (ncx < 3 || ncy < 3 || ncz < 3)) throw ValueError("weno=True needs at least 3 cells per axis");
    const std::vector<int> devs = device_list(device, devices, n_devices);
    auto g = std::make_unique<ttcr_fsm_grid>();
    auto make = [&](int ns, int dev) -> GridBase* {
        GridBase* r;
        if (dtype == TTCR_F32)
            r = new GridT<float>(3, cell_slowness != 0, ncx, ncy, ncz, dx, dx, xmin, ymin, zmin, eps, maxit, ns, translate_origin != 0, dev, weno != 0);
        else
#ifdef FSM_DEV_F32_ONLY   // tuning builds: half the instantiations
            throw ValueError("tuning build without double grids");
#else
            r = new GridT<double>(3, cell_slowness != 0, ncx, ncy, ncz, dx, dx, xmin, ymin, zmin, eps, maxit, ns, translate_origin != 0, dev, weno != 0);
#endif
        r->weno = weno != 0;
        return r;
    };
    g->impl = make_grid(n_slots, devs, make);
    g->impl->weno = weno != 0;
    *out = g.release();
}

static void create2d(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz, double dx, double dz,
                     double xmin, double zmin, double eps, int maxit, int weno, int rotated_template, int n_slots, int device,
                     const int* devices, int n_devices) {
    if (!out) throw ValueError("null output handle");
    *out = nullptr;
    if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
    if (ncx < 1 || ncz < 1) throw ValueError("grid needs at least one cell per axis");
    if (n_slots < 1) throw ValueError("n_slots must be >= 1");
    if (!(dx > 0) || !(dz > 0)) throw ValueError("dx and dz must be positive");
    if (weno && (ncx < 3 || ncz < 3)) throw ValueError("weno=True needs at least 3 cells per axis");
    const std::vector<int> devs = device_list(device, devices, n_devices);
    auto g = std::make_unique<ttcr_fsm_grid>();
    auto make = [&](int ns, int dev) -> GridBase* {
        GridBase* r;
        if (dtype == TTCR_F32)
            r = new GridT<float>(2, cell_slowness != 0, ncx, 0, ncz, dx, dz, xmin, 0.0, zmin, eps, maxit, ns, false, dev, weno != 0);
        else
#ifdef FSM_DEV_F32_ONLY
            throw ValueError("tuning build without double grids");
#else
            r = new GridT<double>(2, cell_slowness != 0, ncx, 0, ncz, dx, dz, xmin, 0.0, zmin, eps, maxit, ns, false, dev, weno != 0);
#endif
        r->weno = weno != 0;
        r->rotated = rotated_template != 0;
        return r;
    };
    g->impl = make_grid(n_slots, devs, make);
    g->impl->weno = weno != 0;
    g->impl->rotated = rotated_template != 0;
    *out = g.release();
}

extern "C" {

int ttcr_fsm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ttcr_fsm_last_error(void) { return g_last_error.c_str(); }

int ttcr_fsm3d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy, uint32_t ncz, double dx,
                      double xmin, double ymin, double zmin, double eps, int maxit, int weno, int n_slots, int translate_origin,
                      int device) {
    return guarded([&] { create3d(out, dtype, cell_slowness, ncx, ncy, ncz, dx, xmin, ymin, zmin, eps, maxit, weno, translate_origin, n_slots, device, nullptr, 0); });
}
int ttcr_fsm3d_create_multi(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy, uint32_t ncz, double dx,
                            double xmin, double ymin, double zmin, double eps, int maxit, int weno, int n_slots, int translate_origin,
                            const int* devices, int n_devices) {
    return guarded([&] {
        if (!devices || n_devices < 1) throw ValueError("device list is empty");
        create3d(out, dtype, cell_slowness, ncx, ncy, ncz, dx, xmin, ymin, zmin, eps, maxit, weno, translate_origin, n_slots, -1, devices, n_devices);
    });
}

int ttcr_fsm2d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz, double dx, double dz,
                      double xmin, double zmin, double eps, int maxit, int weno, int rotated_template, int n_slots, int device) {
    return guarded([&] { create2d(out, dtype, cell_slowness, ncx, ncz, dx, dz, xmin, zmin, eps, maxit, weno, rotated_template, n_slots, device, nullptr, 0); });
}
int ttcr_fsm2d_create_multi(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz, double dx, double dz,
                            double xmin, double zmin, double eps, int maxit, int weno, int rotated_template, int n_slots,
                            const int* devices, int n_devices) {
    return guarded([&] {
        if (!devices || n_devices < 1) throw ValueError("device list is empty");
        create2d(out, dtype, cell_slowness, ncx, ncz, dx, dz, xmin, zmin, eps, maxit, weno, rotated_template, n_slots, -1, devices, n_devices);
    });
}
int ttcr_fsm_n_devices(const ttcr_fsm_grid* g) {
    if (!g) return 0;
    const MultiGrid* m = dynamic_cast<const MultiGrid*>(g->impl.get());
    return m ? (int)m->rep.size() : 1;
}

void ttcr_fsm_destroy(ttcr_fsm_grid* g) { delete g; }

int ttcr_fsm_set_slowness(ttcr_fsm_grid* g, const void* s, size_t n) {
    return guarded_on(g, [&] { g->impl->set_slowness(s, n, false); });
}
int ttcr_fsm_set_slowness_c_order(ttcr_fsm_grid* g, const void* s, size_t n) {
    return guarded_on(g, [&] { g->impl->set_slowness(s, n, false, true); });
}
int ttcr_fsm_set_slowness_device(ttcr_fsm_grid* g, const void* d_s, size_t n) {
    return guarded_on(g, [&] { g->impl->set_slowness(d_s, n, true); });
}
int ttcr_fsm_get_slowness(ttcr_fsm_grid* g, void* out, size_t n) {
    return guarded_on(g, [&] { g->impl->get_slowness(out, n); });
}

// One batch of combined requests (distinct slots): every request is validated on its own (a point outside the grid fails
// that call only), the valid ones go to the device as ONE multi-source solve with their slots, results are copied back.
static void run_combined(GridBase* gb, std::vector<GridBase::Request*>& batch) {
    std::vector<GridBase::Request*> ok;
    for (auto* r : batch) {
        try {
            if (r->slot < 0 || r->slot >= gb->n_slots) throw ValueError("Thread number is larger than number of threads");
            gb->validate_points(r->n_tx, r->tx, r->n_rx, r->rx);
            ok.push_back(r);
        } catch (const ValueError& e) { r->status = TTCR_ERR_VALUE; r->err = e.what();
        } catch (const std::exception& e) { r->status = TTCR_ERR_RUNTIME; r->err = e.what(); }
    }
    if (ok.empty()) return;
    std::sort(ok.begin(), ok.end(), [](const GridBase::Request* a, const GridBase::Request* b) { return a->slot < b->slot; });
    const size_t es = gb->elem_size, nc = gb->dim == 3 ? 3 : 2;
    std::vector<int> tx_off(ok.size() + 1, 0), rx_off(ok.size() + 1, 0), slots(ok.size());
    for (size_t n = 0; n < ok.size(); ++n) {
        tx_off[n + 1] = tx_off[n] + ok[n]->n_tx;
        rx_off[n + 1] = rx_off[n] + std::max(ok[n]->n_rx, 0);
        slots[n] = ok[n]->slot;
    }
    std::vector<char> tx(es * nc * tx_off.back()), t0(es * tx_off.back()), rx(es * nc * std::max(rx_off.back(), 1)), tt(es * std::max(rx_off.back(), 1));
    for (size_t n = 0; n < ok.size(); ++n) {
        std::memcpy(tx.data() + es * nc * tx_off[n], ok[n]->tx, es * nc * ok[n]->n_tx);
        std::memcpy(t0.data() + es * tx_off[n], ok[n]->t0, es * ok[n]->n_tx);
        if (ok[n]->n_rx > 0) std::memcpy(rx.data() + es * nc * rx_off[n], ok[n]->rx, es * nc * ok[n]->n_rx);
    }
    int st = TTCR_OK;
    std::string msg;
    try {
        gb->raytrace_multi((int)ok.size(), tx_off.data(), tx.data(), t0.data(), rx_off.data(), rx.data(), tt.data(), -1, slots.data());
    } catch (const ValueError& e) { st = TTCR_ERR_VALUE; msg = e.what();
    } catch (const DeviceError& e) { st = TTCR_ERR_DEVICE; msg = e.what();
    } catch (const std::exception& e) { st = TTCR_ERR_RUNTIME; msg = e.what(); }
    if (st != TTCR_OK && st != TTCR_ERR_DEVICE && ok.size() > 1) {
        // something only the solve itself finds out (a ray that leaves the grid, ...) failed the batch: the calls are
        // independent in the reference, so each one is redone on its own and only the offending call reports the error
        for (auto* r : ok) {
            const int to[2] = {0, r->n_tx}, ro[2] = {0, std::max(r->n_rx, 0)};
            try {
                gb->raytrace_multi(1, to, r->tx, r->t0, ro, r->rx, r->tt, r->slot);
                r->status = TTCR_OK;
            } catch (const ValueError& e) { r->status = TTCR_ERR_VALUE; r->err = e.what();
            } catch (const DeviceError& e) { r->status = TTCR_ERR_DEVICE; r->err = e.what();
            } catch (const std::exception& e) { r->status = TTCR_ERR_RUNTIME; r->err = e.what(); }
        }
        return;
    }
    for (size_t n = 0; n < ok.size(); ++n) {
        ok[n]->status = st;
        ok[n]->err = msg;
        if (st == TTCR_OK && ok[n]->n_rx > 0) std::memcpy(ok[n]->tt, tt.data() + es * rx_off[n], es * ok[n]->n_rx);
    }
}

int ttcr_fsm_raytrace(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                      void* tt_out) {
    if (!g) { g_last_error = "null grid handle"; return TTCR_ERR_VALUE; }
    GridBase* gb = g->impl.get();
    auto alone = [&] {
        return guarded_on(g, [&] {
            if (slot < 0 || slot >= g->impl->n_slots) throw ValueError("Thread number is larger than number of threads");
            const int tx_off[2] = {0, n_tx}, rx_off[2] = {0, n_rx};
            g->impl->raytrace_multi(1, tx_off, tx, t0, rx_off, rx, tt_out, slot);
        });
    };
    if (gb->n_slots <= 1 || gb->combine_window_us.load() <= 0 || gb->return_rays.load()) return alone();   // (rays belong to "the last call": no company)
    // Grid3D's multi-source overload (ttcr/Grid3D.h:810-853) reaches a backend as nt host threads, each calling the
    // single-source raytrace with its own threadNo.  Calls that arrive within a short window are gathered by the first
    // one (the leader) and go to the device as ONE batch -- the sources then run side by side like in
    // ttcr_fsm_raytrace_multi instead of one after the other.  A handle that has only ever seen one call at a time (a
    // plain loop over sources) never waits for company.
    GridBase::Request req{slot, n_tx, n_rx, tx, t0, rx, tt_out};
    try {
        std::unique_lock<std::mutex> lk(gb->q_mu);
        if (!gb->queue.empty() || gb->leader_active) gb->had_company = true;
        gb->queue.push_back(&req);
        gb->q_cv.notify_all();
        while (!req.done) {
            if (gb->leader_active) { gb->q_cv.wait(lk); continue; }
            gb->leader_active = true;
            std::vector<GridBase::Request*> batch;
            try {
                if (gb->had_company) {
                    const auto window = std::chrono::microseconds(gb->combine_window_us.load());
                    size_t seen = gb->queue.size();
                    while ((int)gb->queue.size() < gb->n_slots) {   // wait for company until nothing new arrives for one window
                        gb->q_cv.wait_for(lk, window);
                        if (gb->queue.size() == seen) break;
                        seen = gb->queue.size();
                    }
                }
                std::vector<GridBase::Request*> rest;
                std::vector<char> taken(gb->n_slots > 0 ? gb->n_slots : 1, 0);
                for (auto* r : gb->queue) {   // one request per slot and batch; a second one for the same slot waits for the next round
                    const bool dup = r->slot >= 0 && r->slot < gb->n_slots && taken[r->slot];
                    if (dup) { rest.push_back(r); continue; }
                    if (r->slot >= 0 && r->slot < gb->n_slots) taken[r->slot] = 1;
                    batch.push_back(r);
                }
                gb->queue.swap(rest);
                lk.unlock();
                try {
                    std::lock_guard<std::mutex> hl(gb->mu);
                    run_combined(gb, batch);
                } catch (...) { lk.lock(); throw; }
                lk.lock();
            } catch (...) {
                // (an allocation failed somewhere above: nobody may be left waiting for a leader that is gone)
                if (batch.empty()) { batch.swap(gb->queue); }
                // (thrown while the batch was being picked: its requests are still queued -- they are marked done below and their
                // callers return, so the queue must not keep pointers to them; remove / erase do not allocate)
                gb->queue.erase(std::remove_if(gb->queue.begin(), gb->queue.end(),
                                               [&](GridBase::Request* q) { return std::find(batch.begin(), batch.end(), q) != batch.end(); }),
                                gb->queue.end());
                for (auto* r : batch)
                    if (r->status == TTCR_OK) { r->status = TTCR_ERR_RUNTIME; r->err = "out of memory while combining raytrace calls"; }
            }
            for (auto* r : batch) r->done = true;
            gb->leader_active = false;
            gb->q_cv.notify_all();
        }
    } catch (...) {
        g_last_error = "out of memory while queueing a raytrace call";
        return TTCR_ERR_RUNTIME;
    }
    if (req.status != TTCR_OK) g_last_error = req.err;
    return req.status;
}

int ttcr_fsm_raytrace_rays(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                           void* tt_out) {
    return guarded_on(g, [&] { g->impl->raytrace_rays(slot, n_tx, tx, t0, n_rx, rx, tt_out); });
}
int ttcr_fsm_raytrace_m(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                        void* tt_out) {
    return guarded_on(g, [&] { g->impl->raytrace_m(slot, n_tx, tx, t0, n_rx, rx, tt_out, false); });
}
int ttcr_fsm_raytrace_rm(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                        void* tt_out) {
    return guarded_on(g, [&] { g->impl->raytrace_m(slot, n_tx, tx, t0, n_rx, rx, tt_out, true); });
}
int ttcr_fsm_raytrace_multi_m(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                              const void* rx, void* tt_out, int with_rays) {
    return guarded_on(g, [&] { g->impl->raytrace_multi_m(n_src, tx_off, tx, t0, rx_off, rx, tt_out, with_rays != 0); });
}
// ---- the M tape (fsm_tape_api.h): owns its device memory and stream, independent of the grid it came from
struct ttcr_fsm_tape {
    int dtype = TTCR_F32;
    ttcr_amd::MTapeDev t;
    std::mutex mu;
    ~ttcr_fsm_tape() { t.release(); }
};

int ttcr_fsm_raytrace_multi_tape(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                 const void* rx, void* tt_out, ttcr_fsm_tape** tape) {
    if (!tape) {
        g_last_error = "null tape output pointer";
        return TTCR_ERR_VALUE;
    }
    *tape = nullptr;
    if (n_src < 0 || (n_src > 0 && (!tx_off || !tx || !t0 || !rx_off || !rx || !tt_out))) {
        g_last_error = "raytrace_multi_tape: null array or negative source count";
        return TTCR_ERR_VALUE;
    }
    return guarded_on(g, [&] {
        GridBase& G = *g->impl;
        ttcr_amd::TapeRows rows;
        G.raytrace_multi_tape(n_src, tx_off, tx, t0, rx_off, rx, tt_out, rows);
        std::unique_ptr<ttcr_fsm_tape> tp(new ttcr_fsm_tape());
        ttcr_amd::MTapeDev& t = tp->t;
        tp->dtype = G.dtype;
        t.device = G.device;
        t.elem = G.elem_size;
        t.n_rows = n_src > 0 ? (size_t)rx_off[n_src] : 0;
        t.nn = G.n_nodes;
        HIP_CHECK(hipSetDevice(t.device));
        HIP_CHECK(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
        if (G.dtype == TTCR_F32) ttcr_amd::tape_finish<float>(t, rows);
        else ttcr_amd::tape_finish<double>(t, rows);
        *tape = tp.release();
    });
}
int ttcr_fsm_tape_size(const ttcr_fsm_tape* t, size_t* n_rows, size_t* n_cols, size_t* nnz) {
    if (!t || !n_rows || !n_cols || !nnz) {
        g_last_error = "null tape or output pointer";
        return TTCR_ERR_VALUE;
    }
    *n_rows = t->t.n_rows;
    *n_cols = t->t.nn;
    *nnz = t->t.nnz;
    return TTCR_OK;
}
int ttcr_fsm_tape_bytes(const ttcr_fsm_tape* t, size_t* bytes) {
    if (!t || !bytes) {
        g_last_error = "null tape or output pointer";
        return TTCR_ERR_VALUE;
    }
    *bytes = t->t.bytes();
    return TTCR_OK;
}
int ttcr_fsm_tape_device(const ttcr_fsm_tape* t, int* device) {
    if (!t || !device) {
        g_last_error = "null tape or output pointer";
        return TTCR_ERR_VALUE;
    }
    *device = t->t.device;
    return TTCR_OK;
}
int ttcr_fsm_tape_get_csr(const ttcr_fsm_tape* t, long long* row_off, long long* j, void* v) {
    if (!t || !row_off || (t->t.nnz > 0 && (!j || !v))) {
        g_last_error = "null tape or output pointer";
        return TTCR_ERR_VALUE;
    }
    ttcr_fsm_tape* tm = const_cast<ttcr_fsm_tape*>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    return guarded([&] {
        const ttcr_amd::MTapeDev& d = t->t;
        HIP_CHECK(hipSetDevice(d.device));
        std::vector<int> col(d.nnz);
        HIP_CHECK(hipMemcpyAsync(row_off, d.row_off, (d.n_rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, d.stream));
        if (d.nnz > 0) {
            HIP_CHECK(hipMemcpyAsync(col.data(), d.col, d.nnz * sizeof(int), hipMemcpyDeviceToHost, d.stream));
            HIP_CHECK(hipMemcpyAsync(v, d.val, d.nnz * d.elem, hipMemcpyDeviceToHost, d.stream));
        }
        HIP_CHECK(hipStreamSynchronize(d.stream));
        for (size_t e = 0; e < d.nnz; ++e) j[e] = col[e];
    });
}
int ttcr_fsm_tape_vjp(const ttcr_fsm_tape* t, const void* w, int w_on_device, void* grad, int grad_on_device) {
    if (!t || (!w && t->t.n_rows > 0) || !grad) {
        g_last_error = "null tape, w or grad";
        return TTCR_ERR_VALUE;
    }
    ttcr_fsm_tape* tm = const_cast<ttcr_fsm_tape*>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    return guarded([&] {
        const ttcr_amd::MTapeDev& d = t->t;
        HIP_CHECK(hipSetDevice(d.device));
        const void* dw = w;
        void* dg = grad_on_device ? grad : d.g_tmp;
        if (!w_on_device) {
            if (d.n_rows > 0) HIP_CHECK(hipMemcpyAsync(d.w_tmp, w, d.n_rows * d.elem, hipMemcpyHostToDevice, d.stream));
            dw = d.w_tmp;
        }
        if (tm->dtype == TTCR_F32) ttcr_amd::tape_vjp<float>(d, (const float*)dw, (float*)dg);
        else ttcr_amd::tape_vjp<double>(d, (const double*)dw, (double*)dg);
        if (!grad_on_device) HIP_CHECK(hipMemcpyAsync(grad, d.g_tmp, d.nn * d.elem, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));
    });
}
int ttcr_fsm_tape_free(ttcr_fsm_tape* t) {
    if (!t) return TTCR_OK;
    return guarded([&] { delete t; });
}
// ---- the field tape (fsm_adjoint_api.h): owns its device memory and stream, independent of the grid it came from
struct ttcr_fsm_adjoint {
    int dtype = TTCR_F32;
    ttcr_amd::AdjTapeDev t;
    std::mutex mu;
    ~ttcr_fsm_adjoint() { t.release(); }
};

// what is wrong with a model shape on a grid of nn3 nodes (null: nothing)
static const char* model_shape_error(const int* model_shape, const int* nn3) {
    if (!model_shape) return "null model_shape";
    for (int d = 0; d < 3; ++d)
        if (model_shape[d] < 1 || model_shape[d] > nn3[d]) return "model_shape: 1 <= m <= the grid's node count on every axis (x, y, z)";
    return nullptr;
}

// the three entries that make a field tape: WRT_CELLS = the cell entry (a cell grid, model vector = cell slowness); WRT_MODEL = the
// model entry (a node grid, model vector = slowness at the nodes of the coarse grid model_shape; model_shape is read for
// that entry only)
static int raytrace_multi_adjoint_entry(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                        const void* rx, void* tt_out, ttcr_fsm_adjoint** tape, TapeWrt wrt, const int* model_shape) {
    const bool wrt_cells = wrt == WRT_CELLS, wrt_model = wrt == WRT_MODEL;
    if (!tape) {
        g_last_error = "null tape output pointer";
        return TTCR_ERR_VALUE;
    }
    *tape = nullptr;
    if (n_src < 0 || (n_src > 0 && (!tx_off || !tx || !t0 || !rx_off || !rx || !tt_out))) {
        g_last_error = wrt_cells ? "raytrace_multi_adjoint_cells: null array or negative source count"
                                 : (wrt_model ? "model_raytrace_multi_adjoint: null array or negative source count"
                                              : "raytrace_multi_adjoint: null array or negative source count");
        return TTCR_ERR_VALUE;
    }
    return guarded_on(g, [&] {
        GridBase& G = *g->impl;
        int nn3[3];
        double spacing = 0;
        G.adjoint_geometry(nn3, &spacing, wrt);
        if (wrt_model)
            if (const char* bad = model_shape_error(model_shape, nn3)) throw ValueError(bad);
        std::unique_ptr<ttcr_fsm_adjoint> tp(new ttcr_fsm_adjoint());
        ttcr_amd::AdjTapeDev& t = tp->t;
        tp->dtype = G.dtype;
        t.device = G.device;
        t.elem = G.elem_size;
        t.n_events = (size_t)n_src;
        t.n_rows = n_src > 0 ? (size_t)rx_off[n_src] : 0;
        t.nn = G.n_nodes;
        t.nnx = nn3[0]; t.nny = nn3[1]; t.nnz = nn3[2];
        t.dx = spacing;
        t.cells = wrt_cells;
        t.nc = wrt_cells ? (size_t)(nn3[0] - 1) * (size_t)(nn3[1] - 1) * (size_t)(nn3[2] - 1) : 0;
        t.model = wrt_model;
        if (wrt_model)
            for (int d = 0; d < 3; ++d) { t.map.n[d] = nn3[d]; t.map.m[d] = model_shape[d]; }
        adj_device_errors([&] {
            HIP_CHECK(hipSetDevice(t.device));
            HIP_CHECK(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
            ttcr_amd::adj_alloc_fields(t);
            ttcr_amd::AdjSink sink;
            sink.device = t.device; sink.elem = t.elem; sink.nn = t.nn; sink.cells = wrt_cells;
            sink.fields = t.fields; sink.slowness = t.slowness;
            sink.fr_node.resize(t.n_events); sink.fr_d.resize(t.n_events);
            sink.fr_pt.resize(t.n_events); sink.fr_c.resize(t.n_events);
            sink.pt_off.assign(tx_off ? tx_off : &n_src, tx_off ? tx_off + n_src + 1 : &n_src + 1);   // (n_src = 0: the one offset 0)
            sink.st_cnt.assign(t.n_rows, 0); sink.st_event.assign(t.n_rows, 0);
            sink.st_node.assign(8 * t.n_rows, 0); sink.st_w.assign(8 * t.n_rows, 0.0);
            sink.st_p.assign(3 * t.n_rows, 0.0);
            G.raytrace_multi_adjoint(n_src, tx_off, tx, t0, rx_off, rx, tt_out, sink);
            HIP_CHECK(hipSetDevice(t.device));
            HIP_CHECK(hipDeviceSynchronize());   // (the replicas of a multi-device grid wrote from their own streams)
            if (G.dtype == TTCR_F32) ttcr_amd::adj_finish<float>(t, sink);
            else ttcr_amd::adj_finish<double>(t, sink);
        });
        *tape = tp.release();
    });
}
int ttcr_fsm_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                    const void* rx, void* tt_out, ttcr_fsm_adjoint** tape) {
    return raytrace_multi_adjoint_entry(g, n_src, tx_off, tx, t0, rx_off, rx, tt_out, tape, WRT_NODES, nullptr);
}
int ttcr_fsm_raytrace_multi_adjoint_cells(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                          const void* rx, void* tt_out, ttcr_fsm_adjoint** tape) {
    return raytrace_multi_adjoint_entry(g, n_src, tx_off, tx, t0, rx_off, rx, tt_out, tape, WRT_CELLS, nullptr);
}
int ttcr_fsm_model_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                          const void* rx, void* tt_out, ttcr_fsm_adjoint** tape, const int model_shape[3]) {
    return raytrace_multi_adjoint_entry(g, n_src, tx_off, tx, t0, rx_off, rx, tt_out, tape, WRT_MODEL, model_shape);
}
// ---- the host layer of the tape's entries: one frame, two staging helpers.
//
// An argument or a result of a product is used in place if it is on the tape's device; a host one goes through a work array of the tape,
// asynchronously on the tape's stream, so that every copy is ordered with the kernels around it.  What is staged where, and why that
// array is free at that moment:
//
//   product                      host argument      staged in     free because
//   ---------------------------  -----------------  ------------  -----------------------------------------------------------------------
//   vjp, hold, vjp_source        w                  w_tmp         nothing else of a vjp uses it (it holds J v in a jvp / Gauss-Newton product)
//                                field_cot          lam2          the Jacobi baseline's second buffer: not in use before the seeds are formed,
//                                                                 and the seeds have read it by then
//                                grad (result)      model_tmp()   written by the last kernel (a cell tape forms the node gradient in
//                                                                 grad_tmp, then A^T into cell_tmp)
//                                gsrc (result)      src_io        allocated by adj_src_prepare, which therefore runs first; no dsrc in a vjp
//   jvp                          ds                 model_tmp()   where a host gradient is staged: no gradient during a jvp
//                                dtt (result)       w_tmp         a jvp has no w
//                                dfields (result)   --            read from the relaxed buffer itself: lam, or lam2 after an odd number of
//                                                                 passes of the Jacobi schedule, which alternates lam -> lam2 -> lam
//   gn, hvp, newton              v and out          model_tmp()   both: v is consumed by the tangent relaxation before the vjp writes the
//                                                                 result to the same place (hvp / newton: the last kernel reads v too;
//                                                                 adj_hess allows d_v == d_out)
//                                row_weight         rw_tmp        part of what the first jvp allocates: adj_jvp_prepare runs before the copy
//   jvp_source                   dsrc               src_io        allocated by adj_src_prepare, which runs first; no gsrc in a jvp
//                                dtt (result)       src_rows      the K-column rows, allocated with src_io
//                                dfields (result)   --            read from the relaxed buffer adj_jvp_source names: as it is for K = 1,
//                                                                 through a host vector that parts the K columns of a node for K = 4
//   jvp_block (per group)        ds                 blk_model     the group's own staging, allocated by adj_block_prepare, which runs first
//                                dtt (result)       blk_rows      a jvp group has no w
//                                dfields (result)   g4            the seeds of a K-column vjp: idle during a jvp
//   vjp_block (per group)        w                  blk_rows      no J v in a vjp group
//                                grad (result)      blk_model     no ds in a vjp group
//   gn_block (per group)         v and out          blk_model     both, as for gn
//                                row_weight         blk_rw        one set shared by the columns: uploaded once, before the loop; a set per
//                                                                 column: the group's columns, uploaded in the loop
//   normal_smooth, normal_dot    v / a, b, out      r, p, q of    the work arrays of the solver's model system (cg[CG_MODEL]): idle outside
//                                                   cg[CG_MODEL]  a solve
//   the three solves             rhs, x0, x         r, x of       not staged but copied, from the host or the device: the solver overwrites
//                                                   cg[system]    r and keeps the iterate in x anyway
//
// The groups of a block product run one after the other on the stream, so a group's staging is free again when the next group's copy is
// enqueued behind it.  Nothing is copied for an empty array, and an argument that is null stays null.
extern "C++" {
// the device pointer to read a `count`-element argument from: `ptr` itself if it is null or on the device, else `staging` after the copy
template <typename T>
static const T* stage_in(ttcr_amd::AdjTapeDev& d, const void* ptr, int on_device, void* staging, size_t count) {
    if (!ptr || on_device) return (const T*)ptr;
    if (count > 0) HIP_CHECK(hipMemcpyAsync(staging, ptr, count * sizeof(T), hipMemcpyHostToDevice, d.stream));
    return (const T*)staging;
}
// the device pointer the kernels write a result to (null if the caller does not want it) ...
template <typename T>
static T* stage_dst(void* dst, int on_device, void* staging) {
    return (T*)(dst && !on_device ? staging : dst);
}
// ... and its way to a host `dst` afterwards
template <typename T>
static void stage_out(ttcr_amd::AdjTapeDev& d, void* dst, int on_device, const void* staging, size_t count) {
    if (dst && !on_device && count > 0) HIP_CHECK(hipMemcpyAsync(dst, staging, count * sizeof(T), hipMemcpyDeviceToHost, d.stream));
}
}  // extern "C++"

static int tape_arg_error(const char* msg) {
    g_last_error = msg;
    return TTCR_ERR_VALUE;
}
static const char* schedule_error(int schedule) {
    return schedule == 0 || schedule == 1 ? nullptr : "schedule: 0 (tiled) or 1 (global Jacobi)";
}

// The frame of every product entry, called once the entry's own argument checks have passed: checks the schedule, locks the tape, turns
// exceptions into a status (the kernel unit's device errors among them), selects the tape's device, calls body(d, T(), p1, p2) with T the
// tape's element type, waits for the tape's stream and hands out the pass counts p1, p2 the body left.  need_held names a product that
// needs a held cotangent.
extern "C++" {
template <typename Body>
static int tape_call(const ttcr_fsm_adjoint* t, int schedule, int* passes1, int* passes2, Body&& body, const char* need_held = nullptr) {
    if (const char* bad = schedule_error(schedule)) return tape_arg_error(bad);
    ttcr_fsm_adjoint* tm = const_cast<ttcr_fsm_adjoint*>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    if (need_held && !tm->t.held) {
        g_last_error = std::string(need_held) + ": the tape holds no cotangent (call ttcr_fsm_adjoint_hold first)";
        return TTCR_ERR_VALUE;
    }
    return guarded([&] {
        adj_device_errors([&] {
            ttcr_amd::AdjTapeDev& d = tm->t;
            HIP_CHECK(hipSetDevice(d.device));
            int p1 = 0, p2 = 0;
            if (tm->dtype == TTCR_F32) body(d, float(), p1, p2);
            else body(d, double(), p1, p2);
            HIP_CHECK(hipStreamSynchronize(d.stream));
            if (passes1) *passes1 = p1;
            if (passes2) *passes2 = p2;
        });
    });
}
// the frame of the release entries: free(d) returns a group of the tape's arrays
template <typename Free>
static int tape_release(ttcr_fsm_adjoint* t, Free&& free) {
    if (!t) return tape_arg_error("null tape");
    std::lock_guard<std::mutex> lock(t->mu);
    return guarded([&] { free(t->t); });
}
}  // extern "C++"

int ttcr_fsm_adjoint_model(const ttcr_fsm_adjoint* t, int* cells, size_t* n_params, size_t* n_nodes) {
    if (!t || !cells || !n_params || !n_nodes) return tape_arg_error("null tape or output pointer");
    *cells = t->t.cells ? 1 : 0;
    *n_params = t->t.n_model();
    *n_nodes = t->t.nn;
    return TTCR_OK;
}
// ---- the coarse model grid
int ttcr_fsm_model_shape(const ttcr_fsm_adjoint* t, int* is_model, int* shape) {
    if (!t || !is_model || !shape) return tape_arg_error("null tape or output pointer");
    *is_model = t->t.model ? 1 : 0;
    for (int d = 0; d < 3; ++d) shape[d] = t->t.model ? t->t.map.m[d] : 0;
    return TTCR_OK;
}
// P and P^T on the tape's stream with the tape's own tables: a host argument goes through cell_tmp (the model vector) or grad_tmp (the
// node vector), which are idle outside a product
static int model_tape_map(const ttcr_fsm_adjoint* t, const void* in, int in_on_device, void* out, int out_on_device, bool prolong) {
    const char* bad = !in ? "null in" : (!out ? "null out" : (!t ? "null tape" : (!t->t.model ? "the tape has no coarse model grid" : nullptr)));
    if (bad) return tape_arg_error(bad);
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        void* st_model = d.cell_tmp;
        void* st_nodes = d.grad_tmp;
        const size_t n_in = prolong ? d.n_model() : d.nn, n_out = prolong ? d.nn : d.n_model();
        const T* din = stage_in<T>(d, in, in_on_device, prolong ? st_model : st_nodes, n_in);
        T* dout = stage_dst<T>(out, out_on_device, prolong ? st_nodes : st_model);
        if (prolong) ttcr_amd::adj_model_to_nodes<T>(d, din, dout);
        else ttcr_amd::adj_nodes_to_model<T>(d, din, dout);
        stage_out<T>(d, out, out_on_device, prolong ? st_nodes : st_model, n_out);
    });
}
int ttcr_fsm_model_tape_prolong(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device) {
    return model_tape_map(t, v, v_on_device, out, out_on_device, true);
}
int ttcr_fsm_model_tape_restrict(const ttcr_fsm_adjoint* t, const void* g, int g_on_device, void* out, int out_on_device) {
    return model_tape_map(t, g, g_on_device, out, out_on_device, false);
}
// ... and on a grid, before any tape exists: tables and intermediates live for the call, on the grid's device and the null stream
extern "C++" {
template <typename T>
static void model_grid_run(const int* nn3, const int* shape, const void* in, int in_on_device, void* out, int out_on_device, bool prolong) {
    ttcr_amd::ModelMap map;
    struct Free {
        ttcr_amd::ModelMap& m;
        ~Free() { ttcr_amd::model_map_free(m); }
    } free_map{map};
    ttcr_amd::model_map_create<T>(map, nn3, shape);
    const size_t n_in = prolong ? map.n_model() : map.n_fine(), n_out = prolong ? map.n_fine() : map.n_model();
    DevBuf<T> b_in, b_out, b_a, b_b;
    const T* din = (const T*)in;
    T* dout = (T*)out;
    if (!in_on_device) {
        b_in.reserve(std::max<size_t>(n_in, 1));
        if (n_in > 0) HIP_CHECK(hipMemcpyAsync(b_in.p, in, n_in * sizeof(T), hipMemcpyHostToDevice, nullptr));
        din = b_in.p;
    }
    if (!out_on_device) {
        b_out.reserve(std::max<size_t>(n_out, 1));
        dout = b_out.p;
    }
    if (prolong) {
        ttcr_amd::model_prolong<T>(map, din, dout, nullptr);
    } else {
        b_a.reserve(std::max<size_t>(map.n_stage_z(), 1));
        b_b.reserve(std::max<size_t>(map.n_stage_y(), 1));
        ttcr_amd::model_restrict<T>(map, din, b_a.p, b_b.p, dout, nullptr);
    }
    if (!out_on_device && n_out > 0) HIP_CHECK(hipMemcpyAsync(out, dout, n_out * sizeof(T), hipMemcpyDeviceToHost, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}
}  // extern "C++"
static int model_grid_map(ttcr_fsm_grid* g, const int* model_shape, const void* in, int in_on_device, void* out, int out_on_device,
                          bool prolong) {
    if (!in || !out) return tape_arg_error(!in ? "null in" : "null out");
    return guarded_on(g, [&] {
        GridBase& G = *g->impl;
        int nn3[3];
        double spacing = 0;
        G.adjoint_geometry(nn3, &spacing, WRT_MODEL);
        if (const char* bad = model_shape_error(model_shape, nn3)) throw ValueError(bad);
        adj_device_errors([&] {
            HIP_CHECK(hipSetDevice(G.device));
            if (G.dtype == TTCR_F32) model_grid_run<float>(nn3, model_shape, in, in_on_device, out, out_on_device, prolong);
            else model_grid_run<double>(nn3, model_shape, in, in_on_device, out, out_on_device, prolong);
        });
    });
}
int ttcr_fsm_model_device(const ttcr_fsm_grid* g, int* device) {
    if (!g || !device) return tape_arg_error(!g ? "null grid handle" : "null device");
    *device = g->impl->device;
    return TTCR_OK;
}
int ttcr_fsm_model_prolong(ttcr_fsm_grid* g, const int model_shape[3], const void* v, int v_on_device, void* out, int out_on_device) {
    return model_grid_map(g, model_shape, v, v_on_device, out, out_on_device, true);
}
int ttcr_fsm_model_restrict(ttcr_fsm_grid* g, const int model_shape[3], const void* gr, int g_on_device, void* out, int out_on_device) {
    return model_grid_map(g, model_shape, gr, g_on_device, out, out_on_device, false);
}
int ttcr_fsm_adjoint_size(const ttcr_fsm_adjoint* t, size_t* n_events, size_t* n_rows, size_t* n_nodes) {
    if (!t || !n_events || !n_rows || !n_nodes) return tape_arg_error("null tape or output pointer");
    *n_events = t->t.n_events;
    *n_rows = t->t.n_rows;
    *n_nodes = t->t.nn;
    return TTCR_OK;
}
int ttcr_fsm_adjoint_bytes(const ttcr_fsm_adjoint* t, size_t* bytes) {
    if (!t || !bytes) return tape_arg_error("null tape or output pointer");
    *bytes = t->t.bytes();
    return TTCR_OK;
}
int ttcr_fsm_adjoint_device(const ttcr_fsm_adjoint* t, int* device) {
    if (!t || !device) return tape_arg_error("null tape or output pointer");
    *device = t->t.device;
    return TTCR_OK;
}
int ttcr_fsm_adjoint_get_field(const ttcr_fsm_adjoint* t, size_t event, void* out) {
    if (!t || !out) return tape_arg_error("null tape or output pointer");
    if (event >= t->t.n_events) return tape_arg_error("event index out of range");
    ttcr_fsm_adjoint* tm = const_cast<ttcr_fsm_adjoint*>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    return guarded([&] {
        const ttcr_amd::AdjTapeDev& d = t->t;
        HIP_CHECK(hipSetDevice(d.device));
        HIP_CHECK(hipMemcpyAsync(out, (const char*)d.fields + event * d.nn * d.elem, d.nn * d.elem, hipMemcpyDeviceToHost, d.stream));
        HIP_CHECK(hipStreamSynchronize(d.stream));
    });
}
int ttcr_fsm_adjoint_points(const ttcr_fsm_adjoint* t, size_t* n_points, int* event_of_point) {
    if (!t || !n_points) return tape_arg_error(!t ? "null tape" : "null n_points");
    *n_points = t->t.n_points;
    if (event_of_point) std::copy(t->t.h_pt_event.begin(), t->t.h_pt_event.end(), event_of_point);
    return TTCR_OK;
}

// vjp, hold and vjp_source: one body.  They differ in the adj_* that runs, in whether grad may be null (the entries check) and in gsrc.
enum TapeBack { TAPE_VJP, TAPE_HOLD, TAPE_VJP_SOURCE };
static int tape_back(const ttcr_fsm_adjoint* t, TapeBack which, const void* w, int w_on_device, const void* field_cot, int fc_on_device,
                     void* grad, int grad_on_device, void* gsrc, int gsrc_on_device, int schedule, int* passes) {
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        if (which == TAPE_VJP_SOURCE) ttcr_amd::adj_src_prepare<T>(d);
        const T* dw = stage_in<T>(d, w, w_on_device, d.w_tmp, d.n_rows);
        const T* dfc = stage_in<T>(d, field_cot, fc_on_device, d.lam2, d.n_events * d.nn);
        T* dg = stage_dst<T>(grad, grad_on_device, d.model_tmp());
        T* dgs = stage_dst<T>(gsrc, gsrc_on_device, d.src_io);
        if (which == TAPE_VJP) np = ttcr_amd::adj_vjp<T>(d, dw, dfc, dg, schedule);
        else if (which == TAPE_HOLD) np = ttcr_amd::adj_hold<T>(d, dw, dfc, dg, schedule);
        else np = ttcr_amd::adj_vjp_source<T>(d, dw, dfc, dg, dgs, schedule);
        stage_out<T>(d, grad, grad_on_device, d.model_tmp(), d.n_model());
        stage_out<T>(d, gsrc, gsrc_on_device, d.src_io, 4 * d.n_points);
    });
}
int ttcr_fsm_adjoint_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                         int grad_on_device, int schedule, int* passes) {
    if (!t || !grad || (!w && !field_cot))
        return tape_arg_error(!t ? "null tape" : (!grad ? "null grad" : "w and field_cot are both null: nothing to back-propagate"));
    return tape_back(t, TAPE_VJP, w, w_on_device, field_cot, fc_on_device, grad, grad_on_device, nullptr, 0, schedule, passes);
}
int ttcr_fsm_adjoint_vjp_source(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                                int grad_on_device, void* gsrc, int gsrc_on_device, int schedule, int* passes) {
    if (!t || !gsrc || (!w && !field_cot))
        return tape_arg_error(!t ? "null tape" : (!gsrc ? "null gsrc" : "w and field_cot are both null: nothing to back-propagate"));
    return tape_back(t, TAPE_VJP_SOURCE, w, w_on_device, field_cot, fc_on_device, grad, grad_on_device, gsrc, gsrc_on_device, schedule,
                     passes);
}
// (second-order products, DESIGN.md 6f: hold keeps the lam of this vjp on the tape)
int ttcr_fsm_adjoint_hold(ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                          int grad_on_device, int schedule, int* passes) {
    if (!t || (!w && !field_cot)) return tape_arg_error(!t ? "null tape" : "w and field_cot are both null: no cotangent to hold");
    return tape_back(t, TAPE_HOLD, w, w_on_device, field_cot, fc_on_device, grad, grad_on_device, nullptr, 0, schedule, passes);
}
int ttcr_fsm_adjoint_release(ttcr_fsm_adjoint* t) { return tape_release(t, ttcr_amd::adj_release_hold); }

int ttcr_fsm_adjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, void* dtt, int dtt_on_device, void* dfields,
                         int df_on_device, int schedule, int* passes) {
    if (!t || !ds || (!dtt && !dfields))
        return tape_arg_error(!t ? "null tape" : (!ds ? "null ds" : "dtt and dfields are both null: nothing to compute"));
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        const T* dds = stage_in<T>(d, ds, ds_on_device, d.model_tmp(), d.n_model());
        np = ttcr_amd::adj_jvp<T>(d, dds, stage_dst<T>(dtt, dtt_on_device, d.w_tmp), df_on_device ? (T*)dfields : nullptr, schedule);
        stage_out<T>(d, dtt, dtt_on_device, d.w_tmp, d.n_rows);
        stage_out<T>(d, dfields, df_on_device, (schedule != 0 && np % 2 == 1) ? d.lam2 : d.lam, d.n_events * d.nn);
    });
}
int ttcr_fsm_adjoint_jvp_source(const ttcr_fsm_adjoint* t, const void* dsrc, int dsrc_on_device, int n_cols, void* dtt, int dtt_on_device,
                                void* dfields, int df_on_device, int schedule, int* passes) {
    if (!t || !dsrc || (!dtt && !dfields))
        return tape_arg_error(!t ? "null tape" : (!dsrc ? "null dsrc" : "dtt and dfields are both null: nothing to compute"));
    if (n_cols < 1 || n_cols > 4) return tape_arg_error("n_cols: 1 to 4 columns per call");
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        const size_t en = d.n_events * d.nn, nc = (size_t)n_cols;
        ttcr_amd::adj_src_prepare<T>(d);
        const T* dd = stage_in<T>(d, dsrc, dsrc_on_device, d.src_io, nc * d.n_points * 4);
        int K = 1;
        const T* mu = nullptr;
        np = ttcr_amd::adj_jvp_source<T>(d, dd, n_cols, stage_dst<T>(dtt, dtt_on_device, d.src_rows), df_on_device ? (T*)dfields : nullptr,
                                         schedule, &mu, &K);
        stage_out<T>(d, dtt, dtt_on_device, d.src_rows, nc * d.n_rows);
        if (K == 1) {
            stage_out<T>(d, dfields, df_on_device, mu, en);
        } else if (dfields && !df_on_device && en > 0) {   // (the K columns of a node are adjacent in the relaxed buffer: parted here)
            std::vector<T> tmp(en * K);
            HIP_CHECK(hipMemcpyAsync(tmp.data(), mu, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, d.stream));
            HIP_CHECK(hipStreamSynchronize(d.stream));
            for (size_t k = 0; k < nc; ++k)
                for (size_t i = 0; i < en; ++i) ((T*)dfields)[k * en + i] = tmp[i * K + k];
        }
    });
}

// The pair weights of a double-difference product, checked behind the tape: pairs have to be set, and a host pair_weight
// holds finite values >= 0 (a device one is the caller's to check).  Null pair_weight: today's diagonal weighting, nothing to check.
static const char* dd_weight_error(const ttcr_fsm_adjoint* t, const void* pair_weight, int pw_on_device) {
    if (!pair_weight) return nullptr;
    if (!t->t.dd_set) return "pair_weight: the tape has no row pairs (call ttcr_fsm_dd_pairs first)";
    if (pw_on_device) return nullptr;
    for (size_t p = 0; p < t->t.n_pairs; ++p) {
        const double w = t->dtype == TTCR_F32 ? (double)((const float*)pair_weight)[p] : ((const double*)pair_weight)[p];
        if (!(w >= 0.0) || !std::isfinite(w)) return "pair_weight: finite values >= 0";
    }
    return nullptr;
}
extern "C++" {
// the row operator of a product: a host row_weight goes through rw_tmp (allocated by adj_jvp_prepare, which therefore runs first), a
// host pair_weight through dd_pw (allocated by adj_dd_prepare, likewise)
template <typename T>
static ttcr_amd::RowOp<T> stage_row_op(ttcr_amd::AdjTapeDev& d, const void* row_weight, int rw_on_device, const void* pair_weight,
                                       int pw_on_device) {
    if (row_weight && !rw_on_device) ttcr_amd::adj_jvp_prepare<T>(d);
    ttcr_amd::RowOp<T> op;
    op.rw = stage_in<T>(d, row_weight, rw_on_device, d.rw_tmp, d.n_rows);
    if (pair_weight) {
        ttcr_amd::adj_dd_prepare(d);
        op.pw = stage_in<T>(d, pair_weight, pw_on_device, d.dd_pw, d.n_pairs);
    }
    return op;
}
}  // extern "C++"

// gn, hvp and newton: one body.  held_for names the product that reads the held cotangent (null: gn); row_weight is null for the hvp.
// pair_weight (null in the entries above 6m): the double-difference rows of ttcr_fsm_dd_gn.
static int tape_normal(const ttcr_fsm_adjoint* t, const char* held_for, bool newton, const void* v, int v_on_device, const void* row_weight,
                       int rw_on_device, void* out, int out_on_device, int schedule, int* passes_jvp, int* passes_vjp,
                       const void* pair_weight = nullptr, int pw_on_device = 0) {
    if (!t || !v || !out) return tape_arg_error(!t ? "null tape" : (!v ? "null v" : "null out"));
    if (const char* bad = dd_weight_error(t, pair_weight, pw_on_device)) return tape_arg_error(bad);
    return tape_call(t, schedule, passes_jvp, passes_vjp, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& pj, int& pv) {
        using T = decltype(tag);
        const T* dv = stage_in<T>(d, v, v_on_device, d.model_tmp(), d.n_model());
        const ttcr_amd::RowOp<T> drw = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);
        T* dout = stage_dst<T>(out, out_on_device, d.model_tmp());
        if (held_for) ttcr_amd::adj_hess<T>(d, dv, drw, newton, dout, schedule, &pj, &pv);
        else ttcr_amd::adj_gn<T>(d, dv, drw, dout, schedule, &pj, &pv);
        stage_out<T>(d, out, out_on_device, d.model_tmp(), d.n_model());
    }, held_for);
}
int ttcr_fsm_adjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device, void* out,
                        int out_on_device, int schedule, int* passes_jvp, int* passes_vjp) {
    return tape_normal(t, nullptr, false, v, v_on_device, row_weight, rw_on_device, out, out_on_device, schedule, passes_jvp, passes_vjp);
}
int ttcr_fsm_adjoint_hvp(ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device, int schedule, int* passes_jvp,
                         int* passes_vjp) {
    return tape_normal(t, "hvp", false, v, v_on_device, nullptr, 0, out, out_on_device, schedule, passes_jvp, passes_vjp);
}
int ttcr_fsm_adjoint_newton(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device, void* out,
                            int out_on_device, int schedule, int* passes_jvp, int* passes_vjp) {
    return tape_normal(t, "newton", true, v, v_on_device, row_weight, rw_on_device, out, out_on_device, schedule, passes_jvp, passes_vjp);
}

// ---- block products of the field tape: n_cols model vectors per call, relaxed in groups of four
// the argument checks the three products share: what needs no tape first, the tape last (null: no message)
static const char* adjoint_block_args(const ttcr_fsm_adjoint* t, int n_cols, const void* in, const char* in_null, bool have_out,
                                      const char* out_null, int schedule) {
    if (n_cols < 1) return "n_cols: at least one column per call";
    if (const char* bad = schedule_error(schedule)) return bad;
    if (!in) return in_null;
    if (!have_out) return out_null;
    if (!t) return "null tape";
    return nullptr;
}
int ttcr_fsm_adjoint_jvp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* ds, int ds_on_device, void* dtt, int dtt_on_device,
                               void* dfields, int df_on_device, int schedule, int* passes) {
    if (const char* bad = adjoint_block_args(t, n_cols, ds, "null ds", dtt || dfields, "dtt and dfields are both null: nothing to compute",
                                             schedule))
        return tape_arg_error(bad);
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_block_prepare<T>(d);
        const size_t en = d.n_events * d.nn, nm = d.n_model(), nr = d.n_rows;
        for (int c0 = 0; c0 < n_cols; c0 += 4) {
            const size_t nc = (size_t)std::min(4, n_cols - c0);
            const T* in = stage_in<T>(d, (const T*)ds + (size_t)c0 * nm, ds_on_device, d.blk_model, nc * nm);
            T* gdtt = dtt ? (T*)dtt + (size_t)c0 * nr : nullptr;   // (the group's columns of the caller's arrays)
            T* gdf = dfields ? (T*)dfields + (size_t)c0 * en : nullptr;
            np += ttcr_amd::adj_jvp_block<T>(d, in, (int)nc, stage_dst<T>(gdtt, dtt_on_device, d.blk_rows),
                                             stage_dst<T>(gdf, df_on_device, d.g4), schedule);
            stage_out<T>(d, gdtt, dtt_on_device, d.blk_rows, nc * nr);
            stage_out<T>(d, gdf, df_on_device, d.g4, nc * en);
        }
    });
}
int ttcr_fsm_adjoint_vjp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* w, int w_on_device, void* grad, int grad_on_device,
                               int schedule, int* passes) {
    if (const char* bad = adjoint_block_args(t, n_cols, w, "null w", grad != nullptr, "null grad", schedule)) return tape_arg_error(bad);
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_block_prepare<T>(d);
        const size_t nm = d.n_model(), nr = d.n_rows;
        for (int c0 = 0; c0 < n_cols; c0 += 4) {
            const size_t nc = (size_t)std::min(4, n_cols - c0);
            const T* in = stage_in<T>(d, (const T*)w + (size_t)c0 * nr, w_on_device, d.blk_rows, nc * nr);
            T* gg = (T*)grad + (size_t)c0 * nm;
            np += ttcr_amd::adj_vjp_block<T>(d, in, (int)nc, stage_dst<T>(gg, grad_on_device, d.blk_model), schedule);
            stage_out<T>(d, gg, grad_on_device, d.blk_model, nc * nm);
        }
    });
}
int ttcr_fsm_adjoint_gn_block(const ttcr_fsm_adjoint* t, int n_cols, const void* v, int v_on_device, const void* row_weight, int rw_cols,
                              int rw_on_device, void* out, int out_on_device, int schedule, int* passes_jvp, int* passes_vjp) {
    const char* bad = nullptr;
    if (n_cols >= 1 && rw_cols != 0 && rw_cols != 1 && rw_cols != n_cols) bad = "rw_cols: 0 (no row_weight), 1 (one set for every column) or n_cols";
    else if (n_cols >= 1 && rw_cols != 0 && !row_weight) bad = "null row_weight with rw_cols != 0";
    else bad = adjoint_block_args(t, n_cols, v, "null v", out != nullptr, "null out", schedule);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, schedule, passes_jvp, passes_vjp, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& pj, int& pv) {
        using T = decltype(tag);
        ttcr_amd::adj_block_prepare<T>(d);
        const size_t nm = d.n_model(), nr = d.n_rows;
        const bool shared = rw_cols == 1;
        const T* drw = shared ? stage_in<T>(d, row_weight, rw_on_device, d.blk_rw, nr) : nullptr;
        for (int c0 = 0; c0 < n_cols; c0 += 4) {
            const size_t nc = (size_t)std::min(4, n_cols - c0);
            const T* in = stage_in<T>(d, (const T*)v + (size_t)c0 * nm, v_on_device, d.blk_model, nc * nm);
            if (rw_cols > 1) drw = stage_in<T>(d, (const T*)row_weight + (size_t)c0 * nr, rw_on_device, d.blk_rw, nc * nr);
            T* gout = (T*)out + (size_t)c0 * nm;
            int gj = 0, gv = 0;
            ttcr_amd::adj_gn_block<T>(d, in, drw, shared ? 0 : nr, (int)nc, stage_dst<T>(gout, out_on_device, d.blk_model), schedule, &gj, &gv);
            pj += gj;
            pv += gv;
            stage_out<T>(d, gout, out_on_device, d.blk_model, nc * nm);
        }
    });
}
int ttcr_fsm_adjoint_block_release(ttcr_fsm_adjoint* t) { return tape_release(t, ttcr_amd::adj_block_release); }

// ---- the solver of the field tape: the smoothing operator, the solver's inner product and the CG solve of the three
// systems (ttcr_amd::CgSystem) -- the model vector alone (normal_*), with the source block behind it (joint_*: 4 n_points values, (t0, x, y,
// z) of every point in call order) or with the receiver block (rjoint_*: 4 n_rcv_points values).  The entries check what needs no tape
// first and the tape last.  Host staging (the table above stage_in continued): the work arrays cg[CG_MODEL] are idle outside a solve, so a
// host v of smooth and the first operand of dot go through its r, the second operand of dot through its p, a host result of smooth
// through its q.  A solve copies its right-hand sides (and x0) into r (and x) of its system's work arrays, which the solver overwrites, and
// reads the result from x; a host row_weight goes through rw_tmp as for gn.  The joint tangents stage like jvp and jvp_source do (ds in
// model_tmp(), the block in src_io or rcv_io, dtt in w_tmp).  The joint Gauss-Newton products part src_io or rcv_io, 16 points' values,
// into four blocks: a host v block, the scale c, fl(c * v block) and a host out block; v and out go through model_tmp().  The scale and
// the damping of a block are settings, not data: host doubles (or NULL), checked here and rounded to the tape's dtype.
static const char* normal_weights_error(const double* w, const char* if_null, const char* if_bad) {
    if (!w) return if_null;
    for (int d = 0; d < 3; ++d)
        if (!(w[d] >= 0.0) || !std::isfinite(w[d])) return if_bad;
    return nullptr;
}
static const char* normal_axes_error(const ttcr_fsm_adjoint* t, const double* weights) {
    return ttcr_amd::adj_smooth_error(t->t, weights);
}
static const char* joint_block_error(const double* v, size_t n, const char* if_bad) {
    for (size_t i = 0; v && i < n; ++i)
        if (!(v[i] >= 0.0) || !std::isfinite(v[i])) return if_bad;
    return nullptr;
}
static bool joint_any(const double* v, size_t n) {
    for (size_t i = 0; v && i < n; ++i)
        if (v[i] != 0.0) return true;
    return false;
}
extern "C++" {
// the doubles of a setting rounded to T and uploaded to dst (the stream is waited for: the host vector leaves scope)
template <typename T>
static void joint_upload(ttcr_amd::AdjTapeDev& d, const double* v, size_t n, void* dst) {
    if (n == 0) return;
    const std::vector<T> h(v, v + n);
    HIP_CHECK(hipMemcpyAsync(dst, h.data(), n * sizeof(T), hipMemcpyHostToDevice, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));
}
}  // extern "C++"


// the extra block of a joint system as its entries name it
struct TapeBlock {
    ttcr_amd::CgSystem sys;
    const char *null_d, *null_v, *null_out, *null_rhs, *null_x, *bad_scale, *bad_damp;
};
static const TapeBlock SOURCE_BLOCK = {ttcr_amd::CG_SOURCE, "null dsrc", "null v_src", "null out_src", "null rhs_src", "null x_src",
                                       "source_scale: finite values >= 0", "source_damp: finite values >= 0"};
static const TapeBlock RCV_BLOCK = {ttcr_amd::CG_RECEIVER, "null drcv", "null v_rcv", "null out_rcv", "null rhs_rcv", "null x_rcv",
                                    "rcv_scale: finite values >= 0", "rcv_damp: finite values >= 0"};
extern "C++" {
// what the products of a block need on the tape, and the 16 points' values a host block is staged in (allocated by that)
template <typename T>
static T* block_prepare(ttcr_amd::AdjTapeDev& d, ttcr_amd::CgSystem sys) {
    if (sys == ttcr_amd::CG_SOURCE) ttcr_amd::adj_src_prepare<T>(d);
    else ttcr_amd::adj_rcv_prepare<T>(d);
    return (T*)(sys == ttcr_amd::CG_SOURCE ? d.src_io : d.rcv_io);
}
}  // extern "C++"

int ttcr_fsm_normal_tile_edge(int dtype) { return ttcr_amd::adj_smooth_tile_edge(dtype == TTCR_F32 ? 4 : 8); }
int ttcr_fsm_normal_smooth(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const double* weights, void* out, int out_on_device) {
    const char* bad = normal_weights_error(weights, "null weights", "weights: three finite values >= 0 (x, y, z)");
    if (!bad) bad =!v ? "null v" : (!out ? "null out" : (!t ? "null tape" : normal_axes_error(t, weights)));
    if (bad) return tape_arg_error(bad);
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_cg_prepare(d, ttcr_amd::CG_MODEL);
        const ttcr_amd::CgWork& w = d.cg[ttcr_amd::CG_MODEL];
        const T* dv = stage_in<T>(d, v, v_on_device, w.r, d.n_model());
        ttcr_amd::adj_smooth<T>(d, dv, weights, stage_dst<T>(out, out_on_device, w.q));
        stage_out<T>(d, out, out_on_device, w.q, d.n_model());
    });
}
int ttcr_fsm_normal_dot(ttcr_fsm_adjoint* t, const void* a, int a_on_device, const void* b, int b_on_device, double* result) {
    if (!a || !b || !result || !t) return tape_arg_error(!a ? "null a" : (!b ? "null b" : (!result ? "null result" : "null tape")));
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_cg_prepare(d, ttcr_amd::CG_MODEL);
        const ttcr_amd::CgWork& w = d.cg[ttcr_amd::CG_MODEL];
        const T* da = stage_in<T>(d, a, a_on_device, w.r, d.n_model());
        const T* db = b == a && b_on_device == a_on_device ? da : stage_in<T>(d, b, b_on_device, w.p, d.n_model());
        *result = ttcr_amd::adj_dot<T>(d, da, db);
    });
}

// The three solves: one check of the arguments, one body.  blk is the extra block of a joint system (null: the model system, the only one
// with x0 and newton); rhs_b, x_b, b_damp and b_scale are the block's arguments.  passes: (jvp, vjp) of every iteration, behind the pair of
// A x0 for the model system.
static int tape_solve(ttcr_fsm_adjoint* t, const TapeBlock* blk, const void* rhs, int rhs_on_device, const void* rhs_b, int rb_on_device,
                      const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                      const double* b_damp, const double* b_scale, const void* x0, int x0_on_device, int maxiter, double rtol, int newton,
                      int schedule, void* x, int x_on_device, void* x_b, int xb_on_device, int* status, int* iterations, double* rho,
                      double* pq, int* passes, const void* pair_weight = nullptr, int pw_on_device = 0) {
    const ttcr_amd::CgSystem sys = blk ? blk->sys : ttcr_amd::CG_MODEL;
    const char* bad = nullptr;
    if (!(smooth >= 0.0) || !std::isfinite(smooth)) bad = "smooth: a finite value >= 0";
    else if (!(damp >= 0.0) || !std::isfinite(damp)) bad = "damp: a finite value >= 0";
    else if (maxiter < 1) bad = "maxiter: at least one iteration";
    else if (!(rtol >= 0.0) || !std::isfinite(rtol)) bad = "rtol: a finite value >= 0";
    else if (newton != 0 && newton != 1) bad = "hessian: 0 (gauss_newton) or 1 (newton)";
    else if (const char* w = normal_weights_error(smooth_weights, "null smooth_weights", "smooth_weights: three finite values >= 0 (x, y, z)"))
        bad = w;
    else if (const char* s = schedule_error(schedule)) bad = s;
    else if (!rhs) bad = "null rhs";
    else if (blk && !rhs_b) bad = blk->null_rhs;
    else if (!x) bad = "null x";
    else if (blk && !x_b) bad = blk->null_x;
    else if (!status || !iterations || !rho || !pq) bad = "null status, iterations, rho or pq";
    else if (!t) bad = "null tape";
    else if (const char* c = joint_block_error(b_scale, t->t.cg_block(sys), blk ? blk->bad_scale : nullptr)) bad = c;
    else if (const char* c = joint_block_error(b_damp, t->t.cg_block(sys), blk ? blk->bad_damp : nullptr)) bad = c;
    else if (smooth != 0.0) bad = normal_axes_error(t, smooth_weights);
    if (!bad) bad = dd_weight_error(t, pair_weight, pw_on_device);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, schedule, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        const size_t nm = d.n_model(), nb = d.cg_block(sys);
        if (sys == ttcr_amd::CG_RECEIVER) ttcr_amd::adj_rcv_prepare<T>(d);
        ttcr_amd::adj_cg_prepare(d, sys);
        const ttcr_amd::CgWork& w = d.cg[sys];
        const ttcr_amd::RowOp<T> drw = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);
        auto copy = [&](void* dst, const void* src, size_t n, hipMemcpyKind kind) {
            if (n > 0) HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), kind, d.stream));
        };
        copy(w.r, rhs, nm, rhs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        copy((T*)w.r + nm, rhs_b, nb, rb_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        if (x0) copy(w.x, x0, nm, x0_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        const bool with_damp = joint_any(b_damp, nb);   // (a term whose factor is 0 everywhere is not evaluated)
        if (b_scale) joint_upload<T>(d, b_scale, nb, w.scale);
        if (with_damp) joint_upload<T>(d, b_damp, nb, w.damp);
        ttcr_amd::NormalOperator op;
        op.smooth = smooth;
        op.damp = damp;
        std::copy(smooth_weights, smooth_weights + 3, op.weights);
        op.newton = newton != 0;
        ttcr_amd::NormalResult res;
        ttcr_amd::adj_solve<T>(d, sys, drw, op, x0 != nullptr, b_scale != nullptr, with_damp, maxiter, rtol, schedule, res);
        copy(x, w.x, nm, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
        copy(x_b, (const T*)w.x + nm, nb, xb_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
        *status = res.status;
        *iterations = res.iterations;
        std::copy(res.rho.begin(), res.rho.end(), rho);
        std::copy(res.pq.begin(), res.pq.end(), pq);
        if (passes && !blk) {
            passes[0] = res.passes0[0];
            passes[1] = res.passes0[1];
            passes += 2;
        }
        if (passes) std::copy(res.passes.begin(), res.passes.end(), passes);
    }, newton == 1 ? "newton" : nullptr);
}
int ttcr_fsm_normal_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* row_weight, int rw_on_device, double smooth,
                          const double* smooth_weights, double damp, const void* x0, int x0_on_device, int maxiter, double rtol,
                          int newton, int schedule, void* x, int x_on_device, int* status, int* iterations, double* rho, double* pq,
                          int* passes) {
    return tape_solve(t, nullptr, rhs, rhs_on_device, nullptr, 0, row_weight, rw_on_device, smooth, smooth_weights, damp, nullptr, nullptr, x0,
                      x0_on_device, maxiter, rtol, newton, schedule, x, x_on_device, nullptr, 0, status, iterations, rho, pq, passes);
}
int ttcr_fsm_joint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_src, int rs_on_device,
                         const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                         const double* source_damp, const double* source_scale, int maxiter, double rtol, int schedule, void* x,
                         int x_on_device, void* x_src, int xs_on_device, int* status, int* iterations, double* rho, double* pq, int* passes) {
    return tape_solve(t, &SOURCE_BLOCK, rhs, rhs_on_device, rhs_src, rs_on_device, row_weight, rw_on_device, smooth, smooth_weights, damp,
                      source_damp, source_scale, nullptr, 0, maxiter, rtol, 0, schedule, x, x_on_device, x_src, xs_on_device, status,
                      iterations, rho, pq, passes);
}
int ttcr_fsm_rjoint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_rcv, int rr_on_device,
                          const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                          const double* rcv_damp, const double* rcv_scale, int maxiter, double rtol, int schedule, void* x,
                          int x_on_device, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq, int* passes) {
    return tape_solve(t, &RCV_BLOCK, rhs, rhs_on_device, rhs_rcv, rr_on_device, row_weight, rw_on_device, smooth, smooth_weights, damp, rcv_damp,
                      rcv_scale, nullptr, 0, maxiter, rtol, 0, schedule, x, x_on_device, x_rcv, xr_on_device, status, iterations, rho, pq,
                      passes);
}
int ttcr_fsm_normal_release(ttcr_fsm_adjoint* t) {
    return tape_release(t, [](ttcr_amd::AdjTapeDev& d) { ttcr_amd::adj_cg_release(d, ttcr_amd::CG_MODEL); });
}
int ttcr_fsm_joint_release(ttcr_fsm_adjoint* t) {
    return tape_release(t, [](ttcr_amd::AdjTapeDev& d) { ttcr_amd::adj_cg_release(d, ttcr_amd::CG_SOURCE); });
}

// The joint tangents: one body.  The source tangent comes from a relaxation of its own, which names the buffer it relaxed in; the
// receiver tangent's fields are adj_jvp's (they do not depend on drcv), in the buffer ttcr_fsm_adjoint_jvp reads them from: lam, or lam2
// after an odd number of passes of the Jacobi schedule.
static int tape_joint_jvp(const ttcr_fsm_adjoint* t, const TapeBlock& blk, const void* ds, int ds_on_device, const void* db, int db_on_device,
                          void* dtt, int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes) {
    if (!ds || !db || (!dtt && !dfields) || !t)
        return tape_arg_error(!ds ? "null ds" : (!db ? blk.null_d : (!t ? "null tape" : "dtt and dfields are both null: nothing to compute")));
    return tape_call(t, schedule, passes, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& np, int&) {
        using T = decltype(tag);
        const bool source = blk.sys == ttcr_amd::CG_SOURCE;
        T* io = block_prepare<T>(d, blk.sys);
        if (!source) ttcr_amd::adj_jvp_prepare<T>(d);
        const T* dds = stage_in<T>(d, ds, ds_on_device, d.model_tmp(), d.n_model());
        const T* dd = stage_in<T>(d, db, db_on_device, io, d.cg_block(blk.sys));
        T* ddtt = stage_dst<T>(dtt, dtt_on_device, d.w_tmp);
        T* ddf = df_on_device ? (T*)dfields : nullptr;
        const T* mu = nullptr;
        if (source) {
            np = ttcr_amd::adj_jvp_joint<T>(d, dds, dd, ddtt, ddf, schedule, &mu);
        } else {
            np = ttcr_amd::adj_jvp_rjoint<T>(d, dds, dd, ddtt, ddf, schedule);
            mu = (const T*)((schedule != 0 && np % 2 == 1) ? d.lam2 : d.lam);
        }
        stage_out<T>(d, dtt, dtt_on_device, d.w_tmp, d.n_rows);
        stage_out<T>(d, dfields, df_on_device, mu, d.n_events * d.nn);
    });
}
int ttcr_fsm_joint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* dsrc, int dsrc_on_device, void* dtt,
                       int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes) {
    return tape_joint_jvp(t, SOURCE_BLOCK, ds, ds_on_device, dsrc, dsrc_on_device, dtt, dtt_on_device, dfields, df_on_device, schedule, passes);
}
int ttcr_fsm_rjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* drcv, int drcv_on_device, void* dtt,
                        int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes) {
    return tape_joint_jvp(t, RCV_BLOCK, ds, ds_on_device, drcv, drcv_on_device, dtt, dtt_on_device, dfields, df_on_device, schedule, passes);
}

// The joint Gauss-Newton products: one body.  The order of the two checks behind the tape differs between the entries and is kept:
// rjoint_gn checks the schedule before rcv_scale, joint_gn leaves the schedule to tape_call and so checks it after source_scale.
static int tape_joint_gn(const ttcr_fsm_adjoint* t, const TapeBlock& blk, const void* v, int v_on_device, const void* v_b, int vb_on_device,
                         const void* row_weight, int rw_on_device, const double* b_scale, void* out, int out_on_device, void* out_b,
                         int ob_on_device, int schedule, int* passes_jvp, int* passes_vjp, const void* pair_weight = nullptr,
                         int pw_on_device = 0) {
    const char* bad = !v ? "null v" : (!v_b ? blk.null_v : (!out ? "null out" : (!out_b ? blk.null_out : (!t ? "null tape" : nullptr))));
    if (!bad && blk.sys == ttcr_amd::CG_RECEIVER) bad = schedule_error(schedule);
    if (!bad) bad = joint_block_error(b_scale, t->t.cg_block(blk.sys), blk.bad_scale);
    if (!bad) bad = dd_weight_error(t, pair_weight, pw_on_device);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, schedule, passes_jvp, passes_vjp, [&](ttcr_amd::AdjTapeDev& d, auto tag, int& pj, int& pv) {
        using T = decltype(tag);
        const size_t nb = d.cg_block(blk.sys);
        T* io = block_prepare<T>(d, blk.sys);
        const T* dv = stage_in<T>(d, v, v_on_device, d.model_tmp(), d.n_model());
        const T* dve = stage_in<T>(d, v_b, vb_on_device, io, nb);
        const ttcr_amd::RowOp<T> drw = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);
        if (b_scale) joint_upload<T>(d, b_scale, nb, io + nb);
        T* dout = stage_dst<T>(out, out_on_device, d.model_tmp());
        T* dob = stage_dst<T>(out_b, ob_on_device, io + 3 * nb);
        const T* dc = b_scale ? io + nb : nullptr;
        if (blk.sys == ttcr_amd::CG_SOURCE) ttcr_amd::adj_gn_joint<T>(d, dv, dve, dc, io + 2 * nb, drw, dout, dob, schedule, &pj, &pv);
        else ttcr_amd::adj_gn_rjoint<T>(d, dv, dve, dc, io + 2 * nb, drw, dout, dob, schedule, &pj, &pv);
        stage_out<T>(d, out, out_on_device, d.model_tmp(), d.n_model());
        stage_out<T>(d, out_b, ob_on_device, io + 3 * nb, nb);
    });
}
int ttcr_fsm_joint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_src, int vs_on_device, const void* row_weight,
                      int rw_on_device, const double* source_scale, void* out, int out_on_device, void* out_src, int os_on_device,
                      int schedule, int* passes_jvp, int* passes_vjp) {
    return tape_joint_gn(t, SOURCE_BLOCK, v, v_on_device, v_src, vs_on_device, row_weight, rw_on_device, source_scale, out, out_on_device,
                         out_src, os_on_device, schedule, passes_jvp, passes_vjp);
}
int ttcr_fsm_rjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_rcv, int vr_on_device, const void* row_weight,
                       int rw_on_device, const double* rcv_scale, void* out, int out_on_device, void* out_rcv, int or_on_device,
                       int schedule, int* passes_jvp, int* passes_vjp) {
    return tape_joint_gn(t, RCV_BLOCK, v, v_on_device, v_rcv, vr_on_device, row_weight, rw_on_device, rcv_scale, out, out_on_device, out_rcv,
                         or_on_device, schedule, passes_jvp, passes_vjp);
}

// ---- derivatives with respect to the receiver points of the field tape.  Host staging (the table above stage_in
// continued): rcv_eval stages the events, host points and host results in rcv_stage (7 n_pts values and n_pts ints: points, gradients,
// traveltimes, events), a buffer of the tape that grows to the largest call and is returned by rcv_release -- its sizes are the caller's,
// not the tape's --; jvp_rcv a host drcv in rcv_io and a host dtt in w_tmp; vjp_rcv a host w in w_tmp and a host grcv in rcv_io.
int ttcr_fsm_rcv_eval(const ttcr_fsm_adjoint* t, size_t n_pts, const void* pts, int pts_on_device, const int* event_of_pt, void* tt,
                              int tt_on_device, void* grad, int grad_on_device) {
    const char* bad = (!tt && !grad) ? "tt and grad are both null: nothing to compute"
                                     : (pts && !event_of_pt ? "null event_of_pt" : (!t ? "null tape" : nullptr));
    if (bad) return tape_arg_error(bad);
    if (pts)
        for (size_t i = 0; i < n_pts; ++i)
            if (event_of_pt[i] < 0 || (size_t)event_of_pt[i] >= t->t.n_events) return tape_arg_error("event_of_pt: an event index out of range");
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        if (!pts) {   // the tape's own rows
            ttcr_amd::adj_rcv_prepare<T>(d);
            ttcr_amd::adj_rcv_eval<T>(d, d.n_rows, nullptr, nullptr, false, tt_on_device ? (T*)tt : nullptr, grad_on_device ? (T*)grad : nullptr);
            stage_out<T>(d, tt, tt_on_device, d.rcv_tt, d.n_rows);
            stage_out<T>(d, grad, grad_on_device, d.rcv_G, 3 * d.n_rows);
            return;
        }
        if (n_pts == 0) return;
        T* sp = (T*)ttcr_amd::adj_rcv_stage(d, 7 * n_pts * sizeof(T) + n_pts * sizeof(int));   // points, gradients, traveltimes, events
        T* sg = sp + 3 * n_pts;
        T* st = sg + 3 * n_pts;
        int* ev = (int*)(st + n_pts);
        HIP_CHECK(hipMemcpyAsync(ev, event_of_pt, n_pts * sizeof(int), hipMemcpyHostToDevice, d.stream));
        const T* dp = stage_in<T>(d, pts, pts_on_device, sp, 3 * n_pts);
        ttcr_amd::adj_rcv_eval<T>(d, n_pts, dp, ev, true, stage_dst<T>(tt, tt_on_device, st), stage_dst<T>(grad, grad_on_device, sg));
        stage_out<T>(d, tt, tt_on_device, st, n_pts);
        stage_out<T>(d, grad, grad_on_device, sg, 3 * n_pts);
    });
}
int ttcr_fsm_rcv_points(ttcr_fsm_adjoint* t, const int* set_point_of_row, size_t set_n_points, size_t* n_points, int* point_of_row,
                        int* differing_rows) {
    if (!t) return tape_arg_error("null tape");
    std::lock_guard<std::mutex> lock(t->mu);
    ttcr_amd::AdjTapeDev& d = t->t;
    if (set_point_of_row) {
        if (set_n_points > ((size_t)1 << 29)) return tape_arg_error("n_points: at most 2^29 receiver points");
        for (size_t r = 0; r < d.n_rows; ++r)
            if (set_point_of_row[r] < 0 || (size_t)set_point_of_row[r] >= set_n_points)
                return tape_arg_error("point_of_row: a receiver point index outside 0 .. n_points - 1");
        int pair[2] = {-1, -1};
        const int st = guarded([&] {
            std::vector<int> first(set_n_points, -1);
            for (size_t r = 0; r < d.n_rows; ++r) {   // rows that share a point: bit-equal coordinates (-0 and +0 differ: compared as bytes)
                int& f = first[set_point_of_row[r]];
                if (f < 0) { f = (int)r; continue; }
                if (std::memcmp(&d.h_rcv_p[3 * (size_t)f], &d.h_rcv_p[3 * r], 3 * sizeof(double)) != 0) {
                    pair[0] = f; pair[1] = (int)r;
                    return;
                }
            }
            ttcr_amd::adj_rcv_set_points(d, set_point_of_row, set_n_points);
        });
        if (st != TTCR_OK) return st;
        if (pair[0] >= 0) {
            if (differing_rows) { differing_rows[0] = pair[0]; differing_rows[1] = pair[1]; }
            g_last_error = "point_of_row: tape rows " + std::to_string(pair[0]) + " and " + std::to_string(pair[1]) +
                           " share a receiver point but their receiver coordinates differ";
            return TTCR_ERR_VALUE;
        }
    }
    if (n_points) *n_points = d.n_rcv_points;
    if (point_of_row) std::copy(d.h_rcv_pt.begin(), d.h_rcv_pt.end(), point_of_row);
    return TTCR_OK;
}
int ttcr_fsm_rcv_jvp(const ttcr_fsm_adjoint* t, const void* drcv, int drcv_on_device, void* dtt, int dtt_on_device) {
    if (!drcv || !dtt || !t) return tape_arg_error(!drcv ? "null drcv" : (!dtt ? "null dtt" : "null tape"));
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_rcv_prepare<T>(d);
        const T* dd = stage_in<T>(d, drcv, drcv_on_device, d.rcv_io, 4 * d.n_rcv_points);
        ttcr_amd::adj_jvp_rcv<T>(d, dd, nullptr, stage_dst<T>(dtt, dtt_on_device, d.w_tmp));
        stage_out<T>(d, dtt, dtt_on_device, d.w_tmp, d.n_rows);
    });
}
int ttcr_fsm_rcv_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, void* grcv, int grcv_on_device) {
    if (!w || !grcv || !t) return tape_arg_error(!w ? "null w" : (!grcv ? "null grcv" : "null tape"));
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_rcv_prepare<T>(d);
        const T* dw = stage_in<T>(d, w, w_on_device, d.w_tmp, d.n_rows);
        ttcr_amd::adj_vjp_rcv<T>(d, dw, stage_dst<T>(grcv, grcv_on_device, d.rcv_io));
        stage_out<T>(d, grcv, grcv_on_device, d.rcv_io, 4 * d.n_rcv_points);
    });
}
int ttcr_fsm_rcv_release(ttcr_fsm_adjoint* t) { return tape_release(t, ttcr_amd::adj_rcv_release); }

// ---- double-difference rows of the field tape.  Host staging (the table above stage_in continued): dd_apply stages a host
// x of Q x and B x in w_tmp and a host y of Q^T y in dd_pw, a host result of Q x in dd_u and a host result of the other two in dd_rows
// (B x forms u in dd_u on its way); a host pair_weight of B x and of the products goes through dd_pw, a host row_weight through rw_tmp as
// for gn.  dd_gn and dd_solve are the bodies of the entries they extend (tape_normal, tape_joint_gn, tape_solve) with pair_weight set.
int ttcr_fsm_dd_pairs(ttcr_fsm_adjoint* t, const int* set_row_a, const int* set_row_b, size_t set_n_pairs, size_t* n_pairs, int* row_a,
                      int* row_b, long long* bad_pair) {
    if (bad_pair) *bad_pair = -1;
    if ((set_row_a == nullptr) != (set_row_b == nullptr)) return tape_arg_error(!set_row_a ? "null set_row_a" : "null set_row_b");
    if (set_row_a && set_n_pairs > (((size_t)1 << 30) - 1)) return tape_arg_error("n_pairs: at most 2^30 - 1 row pairs");
    if (!t) return tape_arg_error("null tape");
    std::lock_guard<std::mutex> lock(t->mu);
    ttcr_amd::AdjTapeDev& d = t->t;
    if (set_row_a) {
        for (size_t p = 0; p < set_n_pairs; ++p) {
            const int a = set_row_a[p], b = set_row_b[p];
            const bool range = a < 0 || b < 0 || (size_t)a >= d.n_rows || (size_t)b >= d.n_rows;
            if (!range && a != b) continue;
            if (bad_pair) *bad_pair = (long long)p;
            g_last_error = "row pairs: pair " + std::to_string(p) + " (tape rows " + std::to_string(a) + ", " + std::to_string(b) + ") " +
                           (range ? "names a row outside 0 .. n_rows - 1" : "joins a row to itself");
            return TTCR_ERR_VALUE;
        }
        const int st = guarded([&] { ttcr_amd::adj_dd_set_pairs(d, set_row_a, set_row_b, set_n_pairs); });
        if (st != TTCR_OK) return st;
    }
    if (n_pairs) *n_pairs = d.n_pairs;
    if (row_a) std::copy(d.h_dd_a.begin(), d.h_dd_a.end(), row_a);
    if (row_b) std::copy(d.h_dd_b.begin(), d.h_dd_b.end(), row_b);
    return TTCR_OK;
}
int ttcr_fsm_dd_apply(const ttcr_fsm_adjoint* t, int mode, const void* x, int x_on_device, const void* row_weight, int rw_on_device,
                      const void* pair_weight, int pw_on_device, void* out, int out_on_device) {
    const char* bad = mode < 0 || mode > 2 ? "mode: 0 (Q x), 1 (Q^T y) or 2 (B x)" : (!x ? "null x" : (!out ? "null out" : nullptr));
    if (!bad && mode != 2 && (row_weight || pair_weight)) bad = "row_weight and pair_weight belong to mode 2 (B x) only";
    if (!bad && !t) bad = "null tape";
    if (!bad && !t->t.dd_set) bad = "the tape has no row pairs (call ttcr_fsm_dd_pairs first)";
    if (!bad) bad = dd_weight_error(t, pair_weight, pw_on_device);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        ttcr_amd::adj_dd_prepare(d);
        const bool from_pairs = mode == 1, to_pairs = mode == 0;
        const T* dx = stage_in<T>(d, x, x_on_device, from_pairs ? d.dd_pw : d.w_tmp, from_pairs ? d.n_pairs : d.n_rows);
        const ttcr_amd::RowOp<T> op = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);   // (null pw: u = d)
        void* staging = to_pairs ? d.dd_u : d.dd_rows;
        ttcr_amd::adj_dd_apply<T>(d, mode, dx, op.rw, op.pw, stage_dst<T>(out, out_on_device, staging));
        stage_out<T>(d, out, out_on_device, staging, to_pairs ? d.n_pairs : d.n_rows);
    });
}
static const char* dd_system_error(int system, int newton) {
    if (system < 0 || system > 2) return "system: 0 (model), 1 (source joint) or 2 (receiver joint)";
    if (newton != 0 && newton != 1) return "newton: 0 (gauss_newton) or 1 (newton)";
    if (newton && system != 0) return "newton: offered for the model system (system 0) only";
    return nullptr;
}
int ttcr_fsm_dd_gn(const ttcr_fsm_adjoint* t, int system, int newton, const void* v, int v_on_device, const void* v_b, int vb_on_device,
                   const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device, const double* b_scale, void* out,
                   int out_on_device, void* out_b, int ob_on_device, int schedule, int* passes_jvp, int* passes_vjp) {
    const char* bad = dd_system_error(system, newton);
    if (!bad && !pair_weight) bad = "null pair_weight";
    if (bad) return tape_arg_error(bad);
    if (system == 0)
        return tape_normal(t, newton ? "newton" : nullptr, newton != 0, v, v_on_device, row_weight, rw_on_device, out, out_on_device, schedule,
                           passes_jvp, passes_vjp, pair_weight, pw_on_device);
    return tape_joint_gn(t, system == 1 ? SOURCE_BLOCK : RCV_BLOCK, v, v_on_device, v_b, vb_on_device, row_weight, rw_on_device, b_scale, out,
                         out_on_device, out_b, ob_on_device, schedule, passes_jvp, passes_vjp, pair_weight, pw_on_device);
}
int ttcr_fsm_dd_solve(ttcr_fsm_adjoint* t, int system, const void* rhs, int rhs_on_device, const void* rhs_b, int rb_on_device,
                      const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device, double smooth,
                      const double* smooth_weights, double damp, const double* b_damp, const double* b_scale, const void* x0,
                      int x0_on_device, int maxiter, double rtol, int newton, int schedule, void* x, int x_on_device, void* x_b,
                      int xb_on_device, int* status, int* iterations, double* rho, double* pq, int* passes) {
    const char* bad = dd_system_error(system, newton);
    if (!bad && system != 0 && x0) bad = "x0: offered for the model system (system 0) only";
    if (!bad && !pair_weight) bad = "null pair_weight";
    if (bad) return tape_arg_error(bad);
    const TapeBlock* blk = system == 0 ? nullptr : (system == 1 ? &SOURCE_BLOCK : &RCV_BLOCK);
    return tape_solve(t, blk, rhs, rhs_on_device, blk ? rhs_b : nullptr, rb_on_device, row_weight, rw_on_device, smooth, smooth_weights, damp,
                      blk ? b_damp : nullptr, blk ? b_scale : nullptr, x0, x0_on_device, maxiter, rtol, newton, schedule, x, x_on_device,
                      blk ? x_b : nullptr, xb_on_device, status, iterations, rho, pq, passes, pair_weight, pw_on_device);
}
int ttcr_fsm_dd_release(ttcr_fsm_adjoint* t) { return tape_release(t, ttcr_amd::adj_dd_release); }

// ---- moving the receiver points of the field tape, and the relocation-only system.  Host staging (the table above
// stage_in continued): rcv_move uploads host points through rcv_io (device points are copied to the host once, for the checks and the
// offsets the host forms) and hands a host tt out of rcv_tt itself; reloc_gn parts rcv_io as the joint products do (a host v block, the
// scale, fl(c * v), a host out block); reloc_solve copies its right-hand side into r of cg[CG_RELOC] and reads x from its x.
int ttcr_fsm_reloc_move(ttcr_fsm_adjoint* t, const void* pts, int pts_on_device, void* tt, int tt_on_device) {
    if (!pts || !t) return tape_arg_error(!pts ? "null pts" : "null tape");
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        const size_t n = d.n_rcv_points;
        std::vector<T> host;
        const T* hp = (const T*)pts;
        if (pts_on_device) {
            host.resize(std::max<size_t>(3 * n, 1));
            if (n > 0) HIP_CHECK(hipMemcpyAsync(host.data(), pts, 3 * n * sizeof(T), hipMemcpyDeviceToHost, d.stream));
            HIP_CHECK(hipStreamSynchronize(d.stream));
            hp = host.data();
        }
        if (const char* bad = ttcr_amd::adj_rcv_move_error<T>(d, hp)) throw ValueError(bad);
        ttcr_amd::adj_rcv_move<T>(d, hp, pts_on_device ? (const T*)pts : nullptr, tt_on_device ? (T*)tt : nullptr);
        stage_out<T>(d, tt, tt_on_device, d.rcv_tt, d.n_rows);
    });
}
int ttcr_fsm_reloc_get_points(const ttcr_fsm_adjoint* t, double* pts) {
    if (!t || !pts) return tape_arg_error(!t ? "null tape" : "null pts");
    ttcr_fsm_adjoint* tm = const_cast<ttcr_fsm_adjoint*>(t);
    std::lock_guard<std::mutex> lock(tm->mu);
    const ttcr_amd::AdjTapeDev& d = t->t;
    if (d.h_mv_pts.size() == 3 * d.n_rcv_points && d.n_rcv_points > 0) {
        std::copy(d.h_mv_pts.begin(), d.h_mv_pts.end(), pts);
        return TTCR_OK;
    }
    const bool f32 = t->dtype == TTCR_F32;
    for (size_t q = 0; q < d.n_rcv_points; ++q) {
        const bool rows = d.h_rcv_off[q + 1] > d.h_rcv_off[q];
        const size_t r = rows ? (size_t)d.h_rcv_rows[d.h_rcv_off[q]] : 0;
        for (int a = 0; a < 3; ++a) {
            if (!rows) pts[3 * q + a] = std::numeric_limits<double>::quiet_NaN();
            else if (f32) pts[3 * q + a] = (double)((float)d.h_rcv_p[3 * r + a] + (float)d.rcv_shift[a]);
            else pts[3 * q + a] = d.h_rcv_p[3 * r + a] + d.rcv_shift[a];
        }
    }
    return TTCR_OK;
}
int ttcr_fsm_reloc_gn(const ttcr_fsm_adjoint* t, const void* v_rcv, int vr_on_device, const void* row_weight, int rw_on_device,
                      const void* pair_weight, int pw_on_device, const double* rcv_scale, void* out_rcv, int or_on_device) {
    const char* bad = !v_rcv ? RCV_BLOCK.null_v : (!out_rcv ? RCV_BLOCK.null_out : (!t ? "null tape" : nullptr));
    if (!bad) bad = joint_block_error(rcv_scale, t->t.cg_block(ttcr_amd::CG_RELOC), RCV_BLOCK.bad_scale);
    if (!bad) bad = dd_weight_error(t, pair_weight, pw_on_device);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        const size_t nb = d.cg_block(ttcr_amd::CG_RELOC);
        T* io = block_prepare<T>(d, ttcr_amd::CG_RECEIVER);
        const T* dve = stage_in<T>(d, v_rcv, vr_on_device, io, nb);
        const ttcr_amd::RowOp<T> drw = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);
        if (rcv_scale) joint_upload<T>(d, rcv_scale, nb, io + nb);
        T* dob = stage_dst<T>(out_rcv, or_on_device, io + 3 * nb);
        ttcr_amd::adj_gn_reloc<T>(d, dve, rcv_scale ? io + nb : nullptr, io + 2 * nb, drw, dob);
        stage_out<T>(d, out_rcv, or_on_device, io + 3 * nb, nb);
    });
}
int ttcr_fsm_reloc_solve(ttcr_fsm_adjoint* t, const void* rhs_rcv, int rr_on_device, const void* row_weight, int rw_on_device,
                         const void* pair_weight, int pw_on_device, const double* rcv_damp, const double* rcv_scale, int maxiter,
                         double rtol, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq) {
    const ttcr_amd::CgSystem sys = ttcr_amd::CG_RELOC;
    const char* bad = nullptr;
    if (maxiter < 1) bad = "maxiter: at least one iteration";
    else if (!(rtol >= 0.0) || !std::isfinite(rtol)) bad = "rtol: a finite value >= 0";
    else if (!rhs_rcv) bad = RCV_BLOCK.null_rhs;
    else if (!x_rcv) bad = RCV_BLOCK.null_x;
    else if (!status || !iterations || !rho || !pq) bad = "null status, iterations, rho or pq";
    else if (!t) bad = "null tape";
    else if (const char* c = joint_block_error(rcv_scale, t->t.cg_block(sys), RCV_BLOCK.bad_scale)) bad = c;
    else if (const char* c = joint_block_error(rcv_damp, t->t.cg_block(sys), RCV_BLOCK.bad_damp)) bad = c;
    if (!bad) bad = dd_weight_error(t, pair_weight, pw_on_device);
    if (bad) return tape_arg_error(bad);
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        const size_t nb = d.cg_block(sys);
        ttcr_amd::adj_rcv_prepare<T>(d);
        ttcr_amd::adj_cg_prepare(d, sys);
        const ttcr_amd::CgWork& w = d.cg[sys];
        const ttcr_amd::RowOp<T> drw = stage_row_op<T>(d, row_weight, rw_on_device, pair_weight, pw_on_device);
        if (nb > 0) HIP_CHECK(hipMemcpyAsync(w.r, rhs_rcv, nb * sizeof(T), rr_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, d.stream));
        const bool with_damp = joint_any(rcv_damp, nb);   // (a term whose factor is 0 everywhere is not evaluated)
        if (rcv_scale) joint_upload<T>(d, rcv_scale, nb, w.scale);
        if (with_damp) joint_upload<T>(d, rcv_damp, nb, w.damp);
        ttcr_amd::NormalResult res;
        ttcr_amd::adj_solve<T>(d, sys, drw, ttcr_amd::NormalOperator(), false, rcv_scale != nullptr, with_damp, maxiter, rtol, 0, res);
        if (nb > 0) HIP_CHECK(hipMemcpyAsync(x_rcv, w.x, nb * sizeof(T), xr_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, d.stream));
        *status = res.status;
        *iterations = res.iterations;
        std::copy(res.rho.begin(), res.rho.end(), rho);
        std::copy(res.pq.begin(), res.pq.end(), pq);
    });
}

// ---- grid-search hypocentre location on the tape's fields.  Host staging (the table above stage_in continued): the picks
// arrive on the host, by hypocentre; offsets (as ints), fields, times, weights (ones for a null pick_weight) and the weight sums go through
// stage_in into loc_work, the three results come back from it through stage_out, and a host volume is formed in loc_vol -- buffers of
// the tape that grow to the largest call and are returned by loc_release: their sizes are the caller's, not the tape's.
int ttcr_fsm_loc_geometry(const ttcr_fsm_adjoint* t, int* nn, double* dx, double* origin) {
    if (!t || !nn || !dx || !origin) return tape_arg_error(!t ? "null tape" : (!nn ? "null nn" : (!dx ? "null dx" : "null origin")));
    const ttcr_amd::AdjTapeDev& d = t->t;
    nn[0] = d.nnx; nn[1] = d.nny; nn[2] = d.nnz;
    *dx = d.dx;
    for (int a = 0; a < 3; ++a) origin[a] = d.rcv_min[a] + d.rcv_shift[a];   // (one of the two is zero)
    return TTCR_OK;
}
int ttcr_fsm_loc_shape(const ttcr_fsm_adjoint* t, int* node_tile, int* hypo_chunk, int* staged) {
    if (!t || !node_tile || !hypo_chunk || !staged) return tape_arg_error("null tape or output pointer");
    ttcr_amd::adj_loc_shape(t->t, node_tile, hypo_chunk, staged);
    return TTCR_OK;
}
int ttcr_fsm_loc_grid(const ttcr_fsm_adjoint* t, size_t n_hypo, const long long* hypo_off, const int* pick_field, const double* pick_time,
                      const double* pick_weight, const int* box, long long* node_out, double* t0_out, double* misfit_out,
                      void* volume_out, int volume_on_device) {
    // (what can be told without the tape first, the tape last but for the field range and the box: ttcr_fsm_rcv_eval's order)
    const char* bad = !hypo_off ? "null hypo_off"
                                : (!node_out ? "null node_out" : (!t0_out ? "null t0_out" : (!misfit_out ? "null misfit_out" : nullptr)));
    if (bad) return tape_arg_error(bad);
    if (n_hypo > ((size_t)1 << 22)) return tape_arg_error("n_hypo: at most 2^22 hypocentres per call");
    if (hypo_off[0] != 0) return tape_arg_error("hypo_off: the first offset is not 0");
    for (size_t q = 0; q < n_hypo; ++q)
        if (hypo_off[q + 1] < hypo_off[q]) return tape_arg_error("hypo_off: the offsets are not ascending");
    const long long n_picks = hypo_off[n_hypo];
    if (n_picks > 0x7fffffffLL) return tape_arg_error("hypo_off: at most 2^31 - 1 picks per call");
    if (n_picks > 0 && (!pick_field || !pick_time)) return tape_arg_error(!pick_field ? "null pick_field" : "null pick_time");
    for (long long k = 0; k < n_picks; ++k) {
        if (!std::isfinite(pick_time[k])) return tape_arg_error("pick_time: a time that is not finite");
        if (pick_weight && !(std::isfinite(pick_weight[k]) && pick_weight[k] >= 0))
            return tape_arg_error("pick_weight: a weight that is negative or not finite");
    }
    if (!t) return tape_arg_error("null tape");
    const ttcr_amd::AdjTapeDev& dev = t->t;
    for (long long k = 0; k < n_picks; ++k)
        if (pick_field[k] < 0 || (size_t)pick_field[k] >= dev.n_events) return tape_arg_error("pick_field: a field index out of range");
    int bx[6] = {0, dev.nnx, 0, dev.nny, 0, dev.nnz};
    if (box)
        for (int a = 0; a < 3; ++a) {
            if (box[2 * a] < 0 || box[2 * a + 1] > bx[2 * a + 1]) return tape_arg_error("box: a node range outside the grid");
            if (box[2 * a] >= box[2 * a + 1]) return tape_arg_error("box: an empty node range");
            bx[2 * a] = box[2 * a];
            bx[2 * a + 1] = box[2 * a + 1];
        }
    const long long n_box = (long long)(bx[1] - bx[0]) * (bx[3] - bx[2]) * (bx[5] - bx[4]);
    if (n_hypo == 0) return TTCR_OK;
    // the picks as the kernels read them (alive until the frame has waited for the stream)
    std::vector<int> off(n_hypo + 1), field(pick_field, pick_field + n_picks);
    std::vector<double> sw(n_hypo), weight((size_t)n_picks, 1.0);
    if (pick_weight) weight.assign(pick_weight, pick_weight + n_picks);
    for (size_t q = 0; q <= n_hypo; ++q) off[q] = (int)hypo_off[q];
    for (size_t q = 0; q < n_hypo; ++q) {
        double s = 0.0;
        for (int k = off[q]; k < off[q + 1]; ++k) s = s + weight[k];
        sw[q] = s;
    }
    return tape_call(t, 0, nullptr, nullptr, [&](ttcr_amd::AdjTapeDev& d, auto tag, int&, int&) {
        using T = decltype(tag);
        const size_t np = (size_t)n_picks, n_vol = n_hypo * (size_t)n_box;
        const ttcr_amd::LocWork w = ttcr_amd::adj_loc_prepare(d, n_hypo, np, n_box);
        double* vol = nullptr;
        if (volume_out) vol = volume_on_device ? (double*)volume_out : ttcr_amd::adj_loc_volume(d, n_vol);
        stage_in<int>(d, off.data(), 0, w.off, n_hypo + 1);
        stage_in<int>(d, field.data(), 0, w.field, np);
        stage_in<double>(d, pick_time, 0, w.time, np);
        stage_in<double>(d, weight.data(), 0, w.weight, np);
        stage_in<double>(d, sw.data(), 0, w.sw, n_hypo);
        ttcr_amd::adj_loc_search<T>(d, w, n_hypo, bx, vol);
        stage_out<long long>(d, node_out, 0, w.node, n_hypo);
        stage_out<double>(d, t0_out, 0, w.t0, n_hypo);
        stage_out<double>(d, misfit_out, 0, w.misfit, n_hypo);
        stage_out<double>(d, volume_out, volume_on_device, vol, n_vol);
    });
}
int ttcr_fsm_loc_release(ttcr_fsm_adjoint* t) { return tape_release(t, ttcr_amd::adj_loc_release); }
int ttcr_fsm_adjoint_free(ttcr_fsm_adjoint* t) {
    if (!t) return TTCR_OK;
    return guarded([&] { delete t; });
}
int ttcr_fsm_raytrace_multi_l(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                              const void* rx, void* tt_out, int with_rays) {
    return guarded_on(g, [&] { g->impl->raytrace_multi_l(n_src, tx_off, tx, t0, rx_off, rx, tt_out, with_rays != 0); });
}
int ttcr_fsm_multi_l_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz) {
    return guarded_on(g, [&] {
        if (!n_rows || !nnz) throw ValueError("null output pointer");
        g->impl->multi_l_size(n_rows, nnz);
    });
}
int ttcr_fsm_get_multi_l(const ttcr_fsm_grid* g, long long* row_off, long long* cell, void* v) {
    return guarded_on(g, [&] { g->impl->get_multi_l(row_off, cell, v); });
}
int ttcr_fsm_multi_m_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz) {
    return guarded_on(g, [&] {
        if (!n_rows || !nnz) throw ValueError("null output pointer");
        g->impl->multi_m_size(n_rows, nnz);
    });
}
int ttcr_fsm_get_multi_m(const ttcr_fsm_grid* g, long long* row_off, long long* j, void* v) {
    return guarded_on(g, [&] { g->impl->get_multi_m(row_off, j, v); });
}
int ttcr_fsm_slot_m_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz) {
    return guarded_on(g, [&] {
        if (!n_rows || !nnz) throw ValueError("null output pointer");
        g->impl->slot_m_size(slot, n_rows, nnz);
    });
}
int ttcr_fsm_get_slot_m(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* j, void* v) {
    return guarded_on(g, [&] { g->impl->get_slot_m(slot, row_off, j, v); });
}
int ttcr_fsm_raytrace_l(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                        void* tt_out, int with_rays) {
    return guarded_on(g, [&] { g->impl->raytrace_l(slot, n_tx, tx, t0, n_rx, rx, tt_out, with_rays != 0); });
}
int ttcr_fsm_slot_l_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz) {
    return guarded_on(g, [&] {
        if (!n_rows || !nnz) throw ValueError("null output pointer");
        g->impl->slot_l_size(slot, n_rows, nnz);
    });
}
int ttcr_fsm_get_slot_l(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* cell, void* v) {
    return guarded_on(g, [&] { g->impl->get_slot_l(slot, row_off, cell, v); });
}
int ttcr_fsm_slot_rays_size(const ttcr_fsm_grid* g, int slot, size_t* n_rays, size_t* n_points) {
    return guarded_on(g, [&] {
        if (!n_rays || !n_points) throw ValueError("null output pointer");
        g->impl->slot_rays_size(slot, n_rays, n_points);
    });
}
int ttcr_fsm_get_slot_rays(const ttcr_fsm_grid* g, int slot, long long* offsets, void* pts) {
    return guarded_on(g, [&] { g->impl->get_slot_rays(slot, offsets, pts); });
}

int ttcr_fsm_raytrace_multi(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0,
                            const int* rx_off, const void* rx, void* tt_out) {
    return guarded_on(g, [&] { g->impl->raytrace_multi(n_src, tx_off, tx, t0, rx_off, rx, tt_out, -1); });
}

int ttcr_fsm_get_tt(ttcr_fsm_grid* g, int slot, void* out, size_t n) {
    return guarded_on(g, [&] { g->impl->get_tt(slot, out, n); });
}
int ttcr_fsm_get_tt_device(ttcr_fsm_grid* g, int slot, void** d_ptr) {
    return guarded_on(g, [&] {
        if (!d_ptr) throw ValueError("null output pointer");
        *d_ptr = g->impl->tt_device(slot);
    });
}
int ttcr_fsm_get_tt_device_view(ttcr_fsm_grid* g, int slot, void** d_ptr, size_t* stride) {
    return guarded_on(g, [&] {
        if (!d_ptr || !stride) throw ValueError("null output pointer");
        *d_ptr = g->impl->tt_device_view(slot, stride);
    });
}
int ttcr_fsm_interp(ttcr_fsm_grid* g, int slot, int n_pts, const void* pts, void* tt_out) {
    return guarded_on(g, [&] { g->impl->interp(slot, n_pts, pts, tt_out); });
}
int ttcr_fsm_compute_slowness(ttcr_fsm_grid* g, int n_pts, const void* pts, int translated, void* out) {
    return guarded_on(g, [&] { g->impl->compute_slowness(n_pts, pts, translated != 0, out); });
}
int ttcr_fsm_get_niter(ttcr_fsm_grid* g, int slot, int* niter, int* niterw) {
    return guarded_on(g, [&] { g->impl->get_niter(slot, niter, niterw); });
}
int ttcr_fsm_get_changes(ttcr_fsm_grid* g, int slot, double* first_order, int n_first, double* weno, int n_weno) {
    return guarded_on(g, [&] {
        if ((n_first > 0 && !first_order) || (n_weno > 0 && !weno) || n_first < 0 || n_weno < 0) throw ValueError("bad output buffers");
        g->impl->get_changes(slot, first_order, n_first, weno, n_weno);
    });
}
int ttcr_fsm_get_reference_changes(ttcr_fsm_grid* g, int slot, double* first_order, int n_first, double* weno, int n_weno) {
    return guarded_on(g, [&] {
        if ((n_first > 0 && !first_order) || (n_weno > 0 && !weno) || n_first < 0 || n_weno < 0) throw ValueError("bad output buffers");
        g->impl->get_reference_changes(slot, first_order, n_first, weno, n_weno);
    });
}
int ttcr_fsm_n_slots(const ttcr_fsm_grid* g) { return g->impl->n_slots; }
size_t ttcr_fsm_n_nodes(const ttcr_fsm_grid* g) { return g->impl->n_nodes; }
size_t ttcr_fsm_n_cells(const ttcr_fsm_grid* g) { return g->impl->n_cells; }

int ttcr_fsm_set_option(ttcr_fsm_grid* g, const char* key, double value) {
    return guarded_on(g, [&] { g->impl->apply_option(std::string(key ? key : ""), value); });
}

int ttcr_fsm_rays_size(const ttcr_fsm_grid* g, size_t* n_rays, size_t* n_points) {
    return guarded_on(g, [&] { g->impl->rays_size(n_rays, n_points); });
}
int ttcr_fsm_get_rays(const ttcr_fsm_grid* g, long long* offsets, void* pts) {
    return guarded_on(g, [&] { g->impl->get_rays(offsets, pts); });
}

int ttcr_fsm_last_timing(const ttcr_fsm_grid* g, ttcr_fsm_timing* out) {
    return guarded_on(g, [&] {
        const Timing& t = g->impl->timing;
        out->sweep_ms = t.sweep_ms;
        out->total_ms = t.total_ms;
        out->kernel_launches = t.launches;
        out->node_updates = t.node_updates;
        out->evaluated_updates = t.evaluated_updates;
        out->iterations = t.iterations;
        out->n_sources = t.n_sources;
    });
}

int ttcr_fsm_stopping_stats(const ttcr_fsm_grid* g, long long* reference_sums, long long* reference_sums_missed, long long* rounds) {
    return guarded_on(g, [&] { g->impl->stopping_stats(reference_sums, reference_sums_missed, rounds); });
}
int ttcr_fsm_prefill_swaps(const ttcr_fsm_grid* g, long long* swaps) {
    return guarded_on(g, [&] { if (swaps) *swaps = g->impl->prefill_swap_count(); });
}
int ttcr_fsm_prefill_inline_fills(const ttcr_fsm_grid* g, long long* fills) {
    return guarded_on(g, [&] { if (fills) *fills = g->impl->prefill_inline_count(); });
}
int ttcr_fsm_reference_change(ttcr_fsm_grid* g, const void* times, const void* field, int parallel, void* out) {
    return guarded_on(g, [&] {
        if (!times || !field || !out) throw ValueError("ttcr_fsm_reference_change: null argument");
        g->impl->reference_change_host(times, field, parallel != 0, out);
    });
}

int ttcr_fsm_last_kernel(const ttcr_fsm_grid* g, char* buf, size_t n) {
    return guarded_on(g, [&] {
        if (!buf || n == 0) throw ValueError("ttcr_fsm_last_kernel: no buffer");
        const std::string k = g->impl->kernel_name();
        std::snprintf(buf, n, "%s", k.c_str());
    });
}

#ifndef TTCR_BUILD_ID
#define TTCR_BUILD_ID "unknown"
#endif
int ttcr_fsm_unit_order(int dim, int dtype, int stage, int by_time, uint32_t nnx, uint32_t nny, uint32_t nnz, uint32_t* out,
                        size_t capacity, size_t* n_units) {
    return guarded([&] {   // (host arithmetic only: no device is looked for)
        if (dim != 2 && dim != 3) throw ValueError("dim must be 2 or 3");
        if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
        if (stage != 0 && stage != 1) throw ValueError("stage must be 0 (first order) or 1 (WENO)");
        if (nnx < 2 || nnz < 2 || (dim == 3 && nny < 2)) throw ValueError("grid needs at least two nodes per axis");
        if (!n_units) throw ValueError("null unit count");
        // F, J, K axes as in the GridT constructor: 3-D x, y, z; 2-D z, x
        const uint32_t NF = dim == 3 ? nnx : nnz, NJ = dim == 3 ? nny : nnx, NK = dim == 3 ? nnz : 1;
        int PJ, PK, C;
        if (dtype == TTCR_F32) {
            PJ = dim == 3 ? TileCfg<float, 3>::PJ : TileCfg<float, 2>::PJ; PK = dim == 3 ? TileCfg<float, 3>::PK : 1;
            C = dim == 3 ? ChunkCfg<float, 3>::C : ChunkCfg<float, 2>::C;
        } else {
            PJ = dim == 3 ? TileCfg<double, 3>::PJ : TileCfg<double, 2>::PJ; PK = dim == 3 ? TileCfg<double, 3>::PK : 1;
            C = dim == 3 ? ChunkCfg<double, 3>::C : ChunkCfg<double, 2>::C;
        }
        const uint64_t npj = ((uint64_t)NJ + PJ - 1) / PJ, npk = ((uint64_t)NK + PK - 1) / PK;
        if (NF >= (1u << 30) || npj >= (1u << 14) || npk >= (1u << 14)) throw ValueError("grid too large for the patch index of the sweep kernel");
        *n_units = (size_t)(npj * npk) * (dim == 3 ? 8 : 4);
        if (!out) return;
        if (capacity < *n_units) throw ValueError("output buffer too small for the units of the launch");
        const std::vector<uint32_t> xs = fsm_xs_order(dim, (int)NF, (int)NJ, (int)NK, PJ, PK, C, stage == 0 ? 1 : 2, by_time != 0,
                                                      fsm_diag_order((int)npj, (int)npk));
        std::copy(xs.begin(), xs.end(), out);
    });
}

int ttcr_fsm_sweep_plan(int dim, int dtype, int weno, uint32_t nnx, uint32_t nny, uint32_t nnz, int n_slots, const char* const* keys,
                        const double* values, int n_options, int wg_cap, int stage, int batch, int layout, char* name, size_t name_len,
                        long long* out) {
    return guarded([&] {   // (host arithmetic only: no device is looked for)
        if (dim != 2 && dim != 3) throw ValueError("dim must be 2 or 3");
        if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
        if (stage != 0 && stage != 1) throw ValueError("stage must be 0 (first order) or 1 (WENO)");
        if (stage == 1 && !weno) throw ValueError("stage 1 needs a grid with the WENO stage");
        if (nnx < 2 || nnz < 2 || (dim == 3 && nny < 2)) throw ValueError("grid needs at least two nodes per axis");
        if (n_slots < 1 || batch < 1 || batch > n_slots) throw ValueError("1 <= batch <= n_slots");
        if (wg_cap < 1) throw ValueError("the workgroup cap must be positive");
        if (layout < -1 || layout > 1) throw ValueError("layout: -1 (default), 0 or 1");
        if (n_options < 0 || (n_options > 0 && (!keys || !values))) throw ValueError("null options");
        if (!name || name_len == 0 || !out) throw ValueError("null output");
        SweepFacts f;
        if (dtype == TTCR_F32) fsm_sweep_tiles<float>(f, dim); else fsm_sweep_tiles<double>(f, dim);
        // F, J, K axes as in the GridT constructor: 3-D x, y, z; 2-D z, x
        f.NF = (int)(dim == 3 ? nnx : nnz); f.NJ = (int)(dim == 3 ? nny : nnx); f.NK = (int)(dim == 3 ? nnz : 1);
        const uint64_t npj = ((uint64_t)f.NJ + f.PJ - 1) / f.PJ, npk = ((uint64_t)f.NK + f.PK - 1) / f.PK;
        if (nnx >= (1u << 30) || nny >= (1u << 30) || nnz >= (1u << 30) || npj >= (1u << 14) || npk >= (1u << 14))
            throw ValueError("grid too large for the patch index of the sweep kernel");
        f.weno = weno != 0;
        f.n_patches = (int)(npj * npk);
        f.nbf = (f.NF + FSM_BRICK - 1) / FSM_BRICK;
        f.cdirty_wpu = fsm_cdirty_wpu(f.NF, f.PJ, f.PK);
        f.n_launch = fsm_tile_launches(f.NF, f.NJ, f.NK, (int)npj, (int)npk, f.BL);
        f.slab_bits = 32 * FSM_SLAB_WORDS; f.cd_words = FSM_CD_WORDS;
        const SweepTuning tune = fsm_sweep_tuning(wg_cap);
        f.opt = fsm_sweep_options();
        for (int q = 0; q < n_options; ++q) {
            const std::string k = keys[q] ? keys[q] : "";
            const double v = values[q];
            if (k == "mode") f.opt.mode = (int)v;
            else if (k == "skip") f.opt.skip = (int)v;
            else if (k == "lone_chunk") { if (v != 8 && v != 16) throw ValueError("option 'lone_chunk': 8 or 16"); f.opt.lone_chunk = (int)v; }
            else if (k == "arith") { if (v != 0 && v != 1 && v != 2) throw ValueError("option 'arith': 0, 1 or 2"); f.opt.arith = (int)v; }
            else if (k == "rotated") f.rot45 = dim == 2 && v != 0;     // (2-D rotated template with dx == dz)
            else if (k == "probe_skip") f.probe_skip = v != 0;         // (state: what a launch in the probe window does now)
            else throw ValueError("unknown option '" + k + "'");
        }
        bool window = false;
        f.NS = fsm_pair_layout(tune, dim, f.weno, n_slots, dim == 3 ? (long long)f.n_patches : 0, &window);
        if (window && layout >= 0) f.NS = layout ? 2 : 1;
        f.stage = stage;
        if (fsm_persistent(f) && batch > (n_slots + f.NS - 1) / f.NS) throw ValueError("more batch entries than slot groups");
        f.batch = batch;
        const SweepPlan p = fsm_sweep_plan(f, tune);
        std::snprintf(name, name_len, "%s", fsm_sweep_name(p).c_str());
        bool have;
#ifdef FSM_DEV_F32_ONLY   // tuning builds: half the instantiations
        have = dtype == TTCR_F32 && sweep_kernel_exists<float>(p);
#else
        have = dtype == TTCR_F32 ? sweep_kernel_exists<float>(p) : sweep_kernel_exists<double>(p);
#endif
        const long long o[12] = {p.arith_needs_xs ? 1 : have ? 0 : 2, (long long)p.wgs, (long long)p.block, (long long)p.dyn_lds, p.tickets, p.launches,
                                 p.chunk, p.skip, p.XS, p.PRE, p.NS, p.AR};
        std::copy(o, o + 12, out);
    });
}

int ttcr_fsm_chunk_dirty_marks(int dtype, int chunk, int dir, int edge_rule, uint32_t nnx, uint32_t nny, uint32_t nnz, int32_t* out, size_t capacity) {
    return guarded([&] {   // (host arithmetic only: no device is looked for)
        if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
        if (chunk != 8 && chunk != 16) throw ValueError("chunk must be 8 or 16 levels");
        if (dir < 0 || dir > 7) throw ValueError("dir must be one of the eight sweep directions");
        if (nnx < 2 || nny < 2 || nnz < 2) throw ValueError("grid needs at least two nodes per axis");
        if (!out) throw ValueError("null output");
        const int PJ = dtype == TTCR_F32 ? TileCfg<float, 3>::PJ : TileCfg<double, 3>::PJ, PK = dtype == TTCR_F32 ? TileCfg<float, 3>::PK : TileCfg<double, 3>::PK;
        const uint64_t n = (uint64_t)nnx * nny * nnz;
        if (n >= (1ull << 31)) throw ValueError("grid too large");
        if (capacity < (size_t)n * 12) throw ValueError("output buffer too small: 12 words per node");
        const int NF = (int)nnx, NJ = (int)nny, NK = (int)nnz, dn = (dir + 1) % 8;
        for (int k = 0; k < NK; ++k)
            for (int j = 0; j < NJ; ++j)
                for (int i = 0; i < NF; ++i) {
                    int32_t* o = out + (((size_t)k * NJ + j) * NF + i) * 12;
                    int m = 0;
                    for (int q = 0; q < 12; ++q) o[q] = -1;
                    fsm_chunk_marks(NF, NJ, NK, PJ, PK, chunk, 1, dn, j, k, i, i, edge_rule != 0, [&](int tj, int tk, int c0, int c1) {
                        if (m == 3) throw std::logic_error("ttcr_fsm_chunk_dirty_marks: a node marks more than three units");
                        o[4 * m] = tj; o[4 * m + 1] = tk; o[4 * m + 2] = c0; o[4 * m + 3] = c1;
                        ++m;
                    });
                }
    });
}

int ttcr_fsm_prefill_slice(int dtype, uint64_t n_el, uint32_t n_tickets, uint32_t ticket, uint64_t* slice_len, uint64_t* begin, uint64_t* end) {
    return guarded([&] {   // (host arithmetic only: no device is looked for)
        if (dtype != TTCR_F32 && dtype != TTCR_F64) throw ValueError("dtype must be TTCR_F32 or TTCR_F64");
        if (n_tickets == 0) throw ValueError("a launch has at least one ticket");
        const size_t slice = fsm_fill_slice_len((size_t)n_el, n_tickets, dtype == TTCR_F32 ? 4 : 2);
        size_t b = 0, e = 0;
        fsm_fill_slice_range((size_t)n_el, slice, ticket, &b, &e);
        if (slice_len) *slice_len = slice;
        if (begin) *begin = b;
        if (end) *end = e;
    });
}

const char* ttcr_fsm_build_id(void) { return TTCR_BUILD_ID; }

}  // extern "C"
