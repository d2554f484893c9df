/* include/ttcr_amd.h -- C ABI of the MI355X-native fast-sweeping (FSM) eikonal solver.
 *
 * This is the drop-in boundary for the rectilinear FSM path of groupeLIAMG/ttcr:
 * every entry point replaces one member of the C++ interface that ttcrpy's Cython
 * layer programs against (src/ttcrpy/rgrid.pxd:30-145 -> ttcr/Grid3D.h, ttcr/Grid2D.h
 * and the Grid{2,3}Dr{n,c}fs leaves).  Paths below are relative to the reference root.
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross the boundary
 * (integer status + ttcr_fsm_last_error()).
 *
 * Conventions (identical to the reference):
 *   - 3-D flat arrays are x-fastest:  n = (k*(ncy+1)+j)*(ncx+1)+i   (ttcr/Grid3Drn.h:2823)
 *     3-D cell arrays:                c = (k*ncy+j)*ncx+i            (ttcr/Grid3Drcfs.h:96-171)
 *   - 2-D flat arrays are z-fastest:  n = i*(ncz+1)+j                (ttcr/Grid2Drn.h:720)
 *     2-D cell arrays:                c = i*ncz+j                    (ttcr/Grid2Drcfs.h:113-137)
 *   - nc* are CELL counts (nodes = cells+1), as in the reference constructors.
 *   - `dtype` selects the reference instantiation: TTCR_F32 <-> <float,uint32_t>,
 *     TTCR_F64 <-> <double,uint32_t>; all `const void*` arrays hold that type.
 *   - a "slot" is the reference's threadNo: a private traveltime field kept on the
 *     device until the next solve in the same slot (ttcr/Node3Dn.h:109-110).
 *   - threads: every entry point that takes a grid locks that grid (one stream, one captured launch
 *     sequence and the pinned / scratch buffers are shared by its slots), so calls on ONE handle from several
 *     host threads are safe.  Single-source ttcr_fsm_raytrace calls that arrive together on a grid with several
 *     slots -- the way Grid3D's multi-source overload reaches a backend: nt host threads, each with its own
 *     threadNo (ttcr/Grid3D.h:810-853) -- are gathered for a short window (option "combine_window_us", default 200)
 *     and solved as ONE device batch, side by side like a ttcr_fsm_raytrace_multi call; every caller gets its own
 *     status and message.  Other calls on one handle run one after the other.  Different handles are independent.
 *     ttcr_fsm_last_error() is per host thread.
 */
#ifndef TTCR_AMD_H
#define TTCR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ttcr_fsm_grid ttcr_fsm_grid; /* opaque */

enum { TTCR_F32 = 0, TTCR_F64 = 1 };

/* status codes; the Python layer maps them to the exceptions the reference raises */
enum {
    TTCR_OK = 0,
    TTCR_ERR_VALUE = 1,       /* bad argument (Python ValueError in rgrid.pyx)            */
    TTCR_ERR_RUNTIME = 2,     /* std::runtime_error / length_error / logic_error -> RuntimeError */
    TTCR_ERR_DEVICE = 3,      /* HIP failure (no silent CPU fallback: the call fails)     */
    TTCR_ERR_UNSUPPORTED = 4  /* feature of the reference interface not built yet         */
};

/* Number of visible HIP devices (0 when none / runtime missing). */
int ttcr_fsm_device_count(void);

/* Message of the last failing call on this thread (also valid when create fails). */
const char* ttcr_fsm_last_error(void);

/* Replaces: Grid3Drnfs<T,uint32_t>::Grid3Drnfs  (ttcr/Grid3Drnfs.h:39-50)  [cell_slowness = 0]
 *           Grid3Drcfs<T,uint32_t>::Grid3Drcfs  (ttcr/Grid3Drcfs.h:41-52)  [cell_slowness = 1]
 * as constructed in src/ttcrpy/rgrid.pyx:217-224, 254-261 (and the _f twins :1917-1954).
 * eps is the per-node tolerance (scaled by the node count like the ctor does, :49),
 * n_slots is the reference's `nt`, device is the HIP device ordinal (-1: current). */
int ttcr_fsm3d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy,
                      uint32_t ncz, double dx, double xmin, double ymin, double zmin, double eps,
                      int maxit, int weno, int n_slots, int translate_origin, int device);

/* Replaces: Grid2Drnfs<T,uint32_t,sxz<T>>::Grid2Drnfs (ttcr/Grid2Drnfs.h:84-95)
 *           Grid2Drcfs<...>::Grid2Drcfs               (ttcr/Grid2Drcfs.h:45-58)
 * as constructed in src/ttcrpy/rgrid.pyx:2962-2966.  rotated_template: Grid2Drn::sweep45
 * (ttcr/Grid2Drn.h:756-794) after every sweep of the first-order solver when dx == dz and weno is
 * off (ttcr/Grid2Drnfs.h:277-286); ignored otherwise, like the reference does. */
int ttcr_fsm2d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz,
                      double dx, double dz, double xmin, double zmin, double eps, int maxit, int weno,
                      int rotated_template, int n_slots, int device);

/* The same grids on SEVERAL devices of one node -- what Grid3D's multi-source overload does with host threads
 * (ttcr/Grid3D.h:810-853; the reference's OpenCL backend keeps one solver per thread slot in one process,
 * ttcr/Grid3Drnfs_OpenCL.h:172-193): one replica of the grid per entry of `devices` (the same ordinal may appear more
 * than once), the slowness replicated, the n_slots traveltime slots divided over the replicas (slot s lives on replica
 * s / ceil(n_slots / n_devices)), the sources of ttcr_fsm_raytrace_multi block-distributed over ALL slots like
 * get_blk_size (ttcr/Grid3D.h:451-465) and every replica driven by its own host thread: no exchange between devices
 * during a solve, results identical to the one-device grid.  Every other entry point takes such a handle unchanged
 * (a slot argument is routed to the replica that owns the slot).  ttcr_fsm3d_create / ttcr_fsm2d_create with
 * device = -1 do the same when the environment variable TTCR_AMD_DEVICES holds a comma-separated device list, so an
 * unmodified caller can be spread over the GPUs of a node.  ttcr_fsm_n_devices: replicas behind a handle (1: plain). */
int ttcr_fsm3d_create_multi(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy,
                            uint32_t ncz, double dx, double xmin, double ymin, double zmin, double eps,
                            int maxit, int weno, int n_slots, int translate_origin, const int* devices, int n_devices);
int ttcr_fsm2d_create_multi(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz,
                            double dx, double dz, double xmin, double zmin, double eps, int maxit, int weno,
                            int rotated_template, int n_slots, const int* devices, int n_devices);
int ttcr_fsm_n_devices(const ttcr_fsm_grid* g);

/* Replaces: `del self.grid` (src/ttcrpy/rgrid.pyx:284-285). */
void ttcr_fsm_destroy(ttcr_fsm_grid* g);

/* Replaces: Grid3Drn::setSlowness (ttcr/Grid3Drn.h:82-89), Grid3Drcfs::setSlowness
 * (ttcr/Grid3Drcfs.h:88-171), Grid2Drn::setSlowness (ttcr/Grid2Drn.h:71-78),
 * Grid2Drcfs::setSlowness (ttcr/Grid2Drcfs.h:98-138).  n must equal the node count
 * (node grids) or the cell count (cell grids), else TTCR_ERR_RUNTIME with the
 * reference's message.  `s` is a host pointer; the _device variant takes a pointer
 * that is already resident in HBM on the grid's device (no PCIe copy).
 * PRECONDITION: every value is finite and >= 0 (0: what set_velocity makes of an infinite velocity).  The values are not
 * checked; what the sweep kernels do with a NaN, an infinity or a negative slowness is undefined.  Inside the precondition the
 * sweeps are tested bit for bit against the reference from subnormal s dx to s dx whose fp32 candidates overflow (nodes then
 * keep the reference's unreached value max()): DESIGN.md section 4, tests/test_range_gpu.py. */
int ttcr_fsm_set_slowness(ttcr_fsm_grid* g, const void* s, size_t n);
int ttcr_fsm_set_slowness_device(ttcr_fsm_grid* g, const void* d_s, size_t n);
/* The same for a 3-D model that lies in host memory as an (nx, ny, nz) array in C order (z fastest) -- what
 * the Python classes receive (src/ttcrpy/rgrid.pyx:532-569 flattens it to x-fastest on the host before
 * Grid3D::setSlowness): uploaded as it lies, permuted on the device.  2-D grids: identical to
 * ttcr_fsm_set_slowness (their flat order is C order already). */
int ttcr_fsm_set_slowness_c_order(ttcr_fsm_grid* g, const void* s, size_t n);

/* Replaces: Grid3Drn::getSlowness (ttcr/Grid3Drn.h:90-97): NODE slowness, n = node count. */
int ttcr_fsm_get_slowness(ttcr_fsm_grid* g, void* out, size_t n);

/* Replaces: Grid3D::raytrace(Tx,t0,Rx,traveltimes,threadNo) (ttcr/Grid3D.h:470-502) ->
 * Grid3Drnfs::raytrace (ttcr/Grid3Drnfs.h:84-155) with tt_from_rp = false, and the 2-D
 * twin Grid2D::raytrace -> Grid2Drnfs::raytrace (ttcr/Grid2Drnfs.h:198-299).
 * tx: n_tx points (3 or 2 coordinates each) forming ONE source, t0: n_tx origin times,
 * rx: n_rx receivers, tt_out: n_rx traveltimes (Grid3Drn::getTraveltime, :794-930).
 * Points outside the grid -> TTCR_ERR_RUNTIME "Error: Point (...) outside grid." */
int ttcr_fsm_raytrace(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx,
                      const void* rx, void* tt_out);

/* Replaces: the multi-source overload Grid3D::raytrace(vector<vector<sxyz>>&...)
 * (ttcr/Grid3D.h:810-853).  Source n owns tx/t0 rows [tx_off[n], tx_off[n+1]) and rx /
 * tt_out rows [rx_off[n], rx_off[n+1]).  Sources are block-distributed over the slots
 * like get_blk_size (ttcr/Grid3D.h:451-465) and solved concurrently on the device. */
int ttcr_fsm_raytrace_multi(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx,
                            const void* t0, const int* rx_off, const void* rx, void* tt_out);

/* Replaces: Grid3Drn::getTT(tt, threadNo) (ttcr/Grid3Drn.h:102-108). n = node count. */
int ttcr_fsm_get_tt(ttcr_fsm_grid* g, int slot, void* out, size_t n);
/* The same field for a consumer on the device (no reference equivalent; the reference only has the host copy above).
 * ttcr_fsm_get_tt_device: pointer to n_nodes CONTIGUOUS values of slot `slot` in the flat order above.  Where every
 *   slot has its own field (one slot; 2-D grids; weno = 1) this is the field itself; on a first-order 3-D grid whose
 *   batches are big enough for source pairs to pay (n_slots x 16x16 column patches of a sweep > 6 144: e.g. 8 slots
 *   at 512^3, 32 at 256^3) the fields of two slots are interleaved in HBM, so the call de-interleaves into a scratch buffer of
 *   the grid: the pointer stays valid until the next ttcr_fsm_get_tt / ttcr_fsm_get_tt_device call or the
 *   destruction of the grid.
 * ttcr_fsm_get_tt_device_view: zero copy.  *d_ptr addresses node 0 of the slot's field where it lies and *stride is
 *   the distance between consecutive nodes in ELEMENTS of the grid dtype -- 1, or 2 for the interleaved layout
 *   T[p/2][node][2], p = the storage the slot's field occupies (p = slot with option "pair_sources" = 0; otherwise a
 *   multi-source call may have given the sources of its batch to each other's storage): always take pointer and stride
 *   from the call; valid until the next raytrace call that solves a source for that slot.  Both stay owned by the grid. */
int ttcr_fsm_get_tt_device(ttcr_fsm_grid* g, int slot, void** d_ptr);
int ttcr_fsm_get_tt_device_view(ttcr_fsm_grid* g, int slot, void** d_ptr, size_t* stride);

/* Replaces: Grid3Drn::getTraveltime(pt, nt) (ttcr/Grid3Drn.h:794-930) / 2-D (:359-414). */
int ttcr_fsm_interp(ttcr_fsm_grid* g, int slot, int n_pts, const void* pts, void* tt_out);

/* Replaces: Grid3Drn::computeSlowness(pt, isTranslated) (ttcr/Grid3Drn.h:2451-2676) and Grid2Drn::computeSlowness(pt)
 * (ttcr/Grid2Drn.h:262-330), what get_s0 of the Python classes calls per source point (src/ttcrpy/rgrid.pyx:824,
 * :3799): the node slowness interpolated at n_pts points (velocity is interpolated instead when the grid was
 * made with interp_vel, 3-D).  translated != 0: the points are already relative to the origin of a grid built with
 * translate_origin.  A point outside the grid -> TTCR_ERR_RUNTIME (the reference reads its arrays unchecked). */
int ttcr_fsm_compute_slowness(ttcr_fsm_grid* g, int n_pts, const void* pts, int translated, void* out);

/* Replaces: get_niter()/get_niterw() (ttcr/Grid3Drnfs.h:56-57); per slot here
 * (the reference keeps one racy value per grid). */
int ttcr_fsm_get_niter(ttcr_fsm_grid* g, int slot, int* niter, int* niterw);
/* The quantity the stopping rule of the driver loop compared with eps * N (ttcr/Grid3Drnfs.h:141-152: `change`), for
 * every sweep-iteration of the last solve of `slot`: first_order[0..n_first) and weno[0..n_weno) (entries beyond the
 * iterations that ran are 0).  Here it is the fp64 sum of the decreases of all nodes over the iteration's sweeps (equal to
 * the reference's sum of |T_old - T_new| in exact arithmetic; the reference adds it up sequentially in T1). */
int ttcr_fsm_get_changes(ttcr_fsm_grid* g, int slot, double* first_order, int n_first, double* weno, int n_weno);
/* The same iterations as the REFERENCE summed them (ttcr/Grid3Drnfs.h:141-152: sequentially, in node order, in T1), for the iterations
 * that were decided with that sum itself (options "stopping_rule", "stopping_shortcuts"); NaN for the others.  A value below eps * N is what `change >= epsilon`
 * saw (:153), bit for bit; one at or above it may have been cut short there (the sum only grows: the decision is taken). */
int ttcr_fsm_get_reference_changes(ttcr_fsm_grid* g, int slot, double* first_order, int n_first, double* weno, int n_weno);

/* Replaces: getNthreads() (ttcr/Grid3D.h) and the node/cell counts of rgrid.pyx:386-404. */
int ttcr_fsm_n_slots(const ttcr_fsm_grid* g);
size_t ttcr_fsm_n_nodes(const ttcr_fsm_grid* g);
size_t ttcr_fsm_n_cells(const ttcr_fsm_grid* g);

/* Tuning / measurement knobs (no reference equivalent):
 *   "fixed_iters"  > 0: run exactly that many sweep-iterations, ignore eps
 *   "max_batch"    sources swept concurrently by one launch sequence (default: n_slots)
 *   "use_graph"    1: the tile-per-launch driver (mode 0) replays its launch sequence from a hipGraph, the persistent drivers
 *                  launch their kernels directly (default); 0: no graphs; 2: graphs for every driver
 *   "stopping_rule" 1 (default): the reference ends a solve when `change`, the SEQUENTIAL sum in T1, in node order, of abs(times[n] -
 *                  T[n]) falls below eps * N (ttcr/Grid3Drnfs.h:141-152; 2-D: ttcr/Grid2Drnfs.h:265-290).  The sweep kernels
 *                  accumulate the same quantity as an fp64 sum of decreases; at 1.3e8 fp32 nodes the reference's sum reads 1-3 %
 *                  low near the threshold, so an iteration whose fp64 change lies within [1/2, 16] x eps * N (fp64 grids: 1e-6
 *                  either side) is decided by the reference's own sum, computed on the device from a snapshot of the field taken
 *                  before the iteration -- exactly, and in parallel (fsm_refsum_* in fsm_kernels.h: while the running sum stays in
 *                  one binade an addition is an integer increment that depends on the sum only through its parity; blocks of
 *                  elements are summarised for either parity and composed in order).  The snapshot is taken whenever the iteration
 *                  before came within 1e3 windows of the threshold, before the first WENO iteration, and always on grids of up to
 *                  2^24 nodes; an iteration that lands in the window without one is decided by the fp64 sum and counted
 *                  (ttcr_fsm_stopping_stats).  0: the fp64 sum alone.  2: as 1 with the sum as ONE chain of additions (the
 *                  round-4 kernel: 0.5 s per 512^3 field; kept as the checker of the parallel form).  tests/test_stopping_rule_gpu.py
 *                  The sum runs over the non-zero terms alone, in node order (zeros add nothing; in the iterations the rule decides
 *                  all but 1e-4 ... 5e-2 of the nodes did not change): one pass writes the terms of the fields that were asked for
 *                  and brings the snapshot up to the current field, a scan and a second pass compact them.
 *   "stopping_shortcuts"  bits (default 3).  1: on 3-D grids whose sweep kernels keep dirty-brick stamps (exact skipping on), those passes
 *                  and the snapshots read only the 16^3 bricks that changed since the snapshot was last right.  2: the ordered pass is left
 *                  out where it cannot change the decision: with M non-zero terms the sequential T1 sum lies within M u / (1 - M u) of the
 *                  exact sum (u the unit roundoff of T1), which the fp64 sum of decreases gives to 2 (nx + ny + nz) u; `change >= epsilon`
 *                  is then decided as the reference decides it, and ttcr_fsm_get_reference_changes has no value (NaN) for that
 *                  iteration.  0: whole fields, every sum (tests, bisecting).  tests/test_stopping_rule_gpu.py
 *   "lone_chunk"   levels per chunk of the 3-D sweep kernels that keep ONE field per workgroup, where the longer chunk is faster (16, default):
 *                  fp32 first-order sweeps of lone sources and of batches below the pairing threshold (512^3: lone source 6.7 instead of
 *                  7.2 ms per sweep-iteration, 4 sources 9.6 instead of 10.6; 256^3 x 4 sources 3.5 instead of 4.3), fp64 first-order
 *                  sweeps of up to four sources (256^3: 7.1 instead of 8.1 ms for one, 9.1 instead of 10.4 for four), the WENO stage of
 *                  one or two sources (256^3: 319 instead of 381 ms per solve, fp64 537 instead of 664).  8: the chunk length of every
 *                  other kernel, everywhere.  The partial order of the node updates and therefore every result is the same; exact
 *                  skipping steps over chunks of that length.  env TTCR_FSM_LONE_CHUNK.  tests/test_lone_chunk_gpu.py,
 *                  profiles/r05/experiment_chunk_length.txt
 *   "arith"        0 (default): the reference's arithmetic -- every result bit-identical to the reference.  1: tolerance-grade local solvers
 *                  in the first-order sweeps of fp32 grids (Grid3Drn::update_node / Grid2Drn::update_node with dx == dz, ttcr/Grid3Drn.h:
 *                  2936-2956, ttcr/Grid2Drn.h:945-950): the same quadratics evaluated in fp32 on differences from the smallest neighbour
 *                  scaled by 1/(s dx), one v_sqrt_f32 per update instead of two correctly rounded fp64 roots (update3_fast / update2_fast,
 *                  fsm_kernels.h).  NOT bit-identical: a result differs from the reference's by an ulp of the traveltime here and there
 *                  (512^3 gradient model: RMS 8e-7 s on traveltimes up to 13 s, north_star's bound is 1e-5 s; iteration counts the same on
 *                  every model tested).  What it buys: a lone 512^3 source 6.6 -> 5.4 ms per sweep-iteration, 64 sources 87 -> 73 ms,
 *                  8 sources 17.2 -> 14.2 ms (profiles/r06).  Whole-iteration launches only ("mode" 2); fp64 grids, the rotated template
 *                  and 2-D grids with dx != dz keep the reference's arithmetic.  Grids WITH the WENO stage (weno = 1, ttcrpy's default)
 *                  keep it in both stages under arith = 1: the WENO iteration amplifies an ulp of difference in the first-order field to
 *                  1e-3 s (the exact WENO stage behind a tolerance-grade first-order stage ends 4e-5 s RMS, 4e-3 s max from the reference:
 *                  profiles/r06/weno_sensitivity.txt) -- only bit-identical input reproduces the reference there.  2: as 1, and both
 *                  stages of grids with the WENO stage as well (weno_axis_fast, solve3_literal_fast): OUTSIDE the 1e-5 s bound (RMS up to
 *                  5e-5 s, max 4e-3 s at 128^3 - 256^3 -- the size of the WENO stage's own response to rounding), for 256^3 solves of
 *                  240 instead of 319 ms (one source) and 423 instead of 762 ms (eight).  env TTCR_FSM_ARITH.  tests/test_arith_mode_gpu.py
 *   "prefill"      a second set of traveltime fields: while a call that restarted every slot runs, a low-priority side stream fills the
 *                  other set with max() (the reference's reinit, ttcr/Grid3Drnfs.h:92-94), and the next call that restarts every
 *                  slot swaps the sets instead of writing n_slots x n_nodes values in front of its first sweep (512^3 x 64: 32 GB,
 *                  6.8 ms).  Calls that restart some slots fill those in place.  1 on, 0 off, -1 (default): on when the fields take
 *                  >= 64 MiB and twice that is at most half the device memory.  env TTCR_FSM_PREFILL.  tests/test_prefill_gpu.py
 *   "prefill_inline"  who fills the other set ("prefill" on).  1: the work units of the call's first sweep launch, each a slice of it with
 *                  plain 16-byte stores as it draws its ticket -- no launch and no workgroup slot of its own, and nothing left for a call
 *                  that comes back at once to wait for.  Only calls that restart every slot, once the other set exists (from the grid's
 *                  second such call on), with whole-iteration launches ("mode" 2) that are not replayed from a graph ("use_graph" < 2);
 *                  every other call keeps the side stream.  0: always the side stream.  -1 (default): as 1 for 3-D launches of at least
 *                  2 048 work units per sweep (the ones bound by throughput, where exact skipping is on) with the reference's arithmetic
 *                  ("arith" 0), as 0 below and for the tolerance-grade kernels (512^3 x 64: 182.0 -> 179.1 ms per step; with "arith" 1
 *                  147.5 -> 148.5 ... 149.4, profiles/inline_prefill).  Same results either way.  tests/test_inline_prefill_gpu.py
 *   "pair_sources" 1 (default): where the grid keeps its fields in pairs (n_slots x patches of a sweep > 6 144, env
 *                  TTCR_FSM_PAIR_UNITS; TTCR_FSM_PAIR = 1 / 0 forces / forbids the pair layout at grid creation) the sources
 *                  of a batch are paired by distance before they share a workgroup two by two
 *   "pair_layout"  grids whose slots x patches lie between the pairing threshold and 2.5 x that (512^3 nodes: 8 ... 15 slots) change their
 *                  field layout between calls that restart every slot: pairs while the call before evaluated more than 0.45 of its node
 *                  updates (rough models: 311 against 360 ms per solve of 8 sources), one field per workgroup on 16-level chunks once it
 *                  evaluated less (smooth models: 31.5 against 35.5 ms per step), back to pairs above 0.55.  -1 (default): that rule;
 *                  0 / 1: one field per workgroup / pairs, always.  Results do not depend on the layout.  tests/test_pair_layout_gpu.py
 *   "combine_window_us"  single-source calls from several host threads wait this long for one another before they go
 *                  to the device as one batch (default 200; 0: every call on its own)
 *   "mode"         2: persistent sweep kernel, ONE launch per sweep-iteration: patches ordered by
 *                     progress counters in HBM, the next directional sweep starts on the patches the
 *                     previous one has finished (default); 1: same kernel, one launch per directional
 *                     sweep; 0: one launch per tile wavefront.  All three give bit-identical fields.
 *                  (env TTCR_FSM_MODE overrides the default at grid creation)
 *   "tt_from_rp"   1: receiver traveltimes are integrated along the ray traced back through the
 *                     traveltime field (replaces setTraveltimeFromRaypath(bool), ttcr/Grid3D.h, and the
 *                     `ttrp` constructor argument; Grid3Drn::getTraveltimeFromRaypath, ttcr/Grid3Drn.h:
 *                     1103-1243; 2-D: Grid2Drn::getTraveltimeFromRaypath, ttcr/Grid2Drn.h:1478-1661);
 *                     0: tri/bilinear interpolation (getTraveltime).  Default 0.
 *   "interp_vel"   1: the ray integration interpolates velocity instead of slowness (`intVel`
 *                     constructor argument / processVel, ttcr/Grid3Drn.h:2451-2676).  Default 0.
 *   "pair_sources" 1 (default): the sources of a ttcr_fsm_raytrace_multi batch are paired by distance before they share
 *                     the sweep kernel two by two (first-order 3-D grids): the field of the source the block distribution
 *                     gives to thread t may then LIVE in another slot's storage, every entry point that takes a slot
 *                     looks it up, and a caller sees what it would see without (same fields, iteration counts, receivers
 *                     under the same thread numbers).  0: every source in the storage of its own thread number.
 *   "return_rays"  1: the raytrace calls follow the overloads with r_data (Grid3D::raytrace(Tx,t0,Rx,tt,
 *                     r_data,threadNo), ttcr/Grid3D.h:546-586): receiver traveltimes AND raypaths come from
 *                     Grid3Drn::getRaypath(Tx,t0,Rx,r_data,tt,threadNo) (ttcr/Grid3Drn.h:1339-1500); the rays
 *                     stay in the grid until the next raytrace call, see ttcr_fsm_get_rays (2-D: Grid2Drn::
 *                     getRaypath, ttcr/Grid2Drn.h:1663-1850, points are (x, z) pairs).
 *   "walk_records" room of one row of the recording ray walks (return_rays, compute_M, the M tape, compute_L), in records: it takes
 *                     the place of 8 * (ncx + ncy + ncz + 3) (2-D: 8 * (ncx + ncz + 3)) in the row length; the rows of a launch share
 *                     a fixed budget, so a larger value also means fewer receivers per launch.  A walk that needs more than a row is
 *                     walked again alone with the room it asked for.  A buffer size, not arithmetic: no result depends on it (tests
 *                     reach the second walk and the seams between launches with it on small grids).  0 (default): that formula;
 *                     1 ... 1 000 000 (the step limit of a walk); anything else is refused.
 *   "skip"         1: the persistent kernels step over chunks, work units and whole sweeps that cannot change a node:
 *                     a chunk whose read set (bricks of 16^3 nodes stamped with the sweep of their last change; the
 *                     change flags its upwind patches publish with their progress) holds no change since its nodes
 *                     were last visited is a no-op, and so is every sweep that follows a sweep without a change --
 *                     exact, fields and iteration counts are unchanged; 0: evaluate every chunk; -1 (default): on
 *                     where it was measured to pay (2-D grids, the WENO stage, first-order 3-D batches with at least 2048 work
 *                     units per sweep); fp32 first-order 3-D launches of 1024 ... 2047 units (a lone 512^3 source) follow the model:
 *                     skipping while the grid's last skipping solve evaluated less than 0.6 of its node updates (smooth models: 13.3 ->
 *                     12.8 ms per solve), everything evaluated above that (rough models lose 4 - 9 % with it), tried again after eight
 *                     solves; smaller launches never skip.  DESIGN.md 4a, profiles/r06/lone_skip_models.txt */
int ttcr_fsm_set_option(ttcr_fsm_grid* g, const char* key, double value);

/* Replaces: the r_data output of the raytrace overloads above (std::vector<std::vector<sxyz<T1>>>&,
 * src/ttcrpy/rgrid.pxd:60-75).  After a raytrace call with option "return_rays" = 1: one ray per receiver
 * row of that call, in row order; ray n is points [offsets[n], offsets[n+1]) of pts (x,y,z triples -- x,z pairs in 2-D -- of the
 * grid's dtype), from the receiver to the source.  Two calls: sizes first, then the copy into caller
 * buffers of n_rays+1 offsets and 3*n_points (2-D: 2*n_points) coordinates. */
int ttcr_fsm_rays_size(const ttcr_fsm_grid* g, size_t* n_rays, size_t* n_points);
int ttcr_fsm_get_rays(const ttcr_fsm_grid* g, long long* offsets, void* pts);

/* Replaces: Grid3D::raytrace(Tx, t0, Rx, traveltimes, r_data, threadNo) (ttcr/Grid3D.h:546-586; 2-D: ttcr/Grid2D.h) as
 * Grid3D's multi-source r_data overload calls it -- from nt host threads at once, each with its own threadNo
 * (ttcr/Grid3D.h:855-905).  One call solves the source in `slot` and keeps traveltimes AND rays, whatever the
 * "return_rays" option says; the rays are stored PER SLOT, so a thread finds the rays of its own call with
 * ttcr_fsm_slot_rays_size / ttcr_fsm_get_slot_rays (same layout as ttcr_fsm_get_rays) whatever other threads do on other
 * slots meanwhile.  They stay until the next ttcr_fsm_raytrace_rays call on that slot. */
int ttcr_fsm_raytrace_rays(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx,
                           const void* rx, void* tt_out);
int ttcr_fsm_slot_rays_size(const ttcr_fsm_grid* g, int slot, size_t* n_rays, size_t* n_points);
int ttcr_fsm_get_slot_rays(const ttcr_fsm_grid* g, int slot, long long* offsets, void* pts);

/* Replaces: Grid3D::raytrace(Tx, t0, Rx, traveltimes, m_data, threadNo) (ttcr/Grid3D.h:743-772) -> Grid3Drn::getRaypath(Tx,
 * t0, Rx, m_data, RxNo, tt, threadNo) (ttcr/Grid3Drn.h:1503-1800): what `compute_M=True` of the Python layer reaches
 * (src/ttcrpy/rgrid.pyx:1059, :1171-1191).  One call solves the source in `slot`, walks every receiver's ray on the device
 * with the walk of THAT overload (a kernel of its own) and assembles, per receiver, the (node index, value) entries of the
 * matrix of traveltime derivatives in the order the reference pushes them; traveltimes are those of that overload
 * (integrated along the ray; 0 for a receiver on the source).  The reference's formula is restated AS IT STANDS: it
 * overwrites prev_pt with curr_pt before it forms a segment's mid-point and length (:1590-1597), so every step of the walk
 * contributes signed zeros at the eight nodes around the step's end point and only the last hop (or two) to each source point
 * within a cell diagonal carries weight; its weights drop xmin and its node indices may lie one node past the grid (the
 * Python layer drops those).  Bit-identical to the compiled reference (tests/golden/m_golden.npz, tests/test_m_matrix.py),
 * sources of several points -- closely spaced ones included -- as well.  3-D node grids (TTCR_ERR_UNSUPPORTED otherwise, like
 * the Python layer).
 * ttcr_fsm_raytrace_rm replaces the overload that keeps the rays too, Grid3D::raytrace(Tx, t0, Rx, traveltimes, r_data, m_data,
 * threadNo) (ttcr/Grid3D.h:646-680) -> Grid3Drn::getRaypath(Tx, t0, Rx, r_data, m_data, RxNo, tt, threadNo) (ttcr/Grid3Drn.h:
 * 2144-2470), what `compute_M=True, return_rays=True` reaches (rgrid.pyx:1050).  NOT the same matrix: this overload takes
 * prev_pt before it pushes the point, so its segments carry their lengths (one exception, restated as well: the plane point
 * between the walk and a source point, :2359-2366).  The rays of the call: ttcr_fsm_slot_rays_size / ttcr_fsm_get_slot_rays.
 * ttcr_fsm_slot_m_size: rows (= receivers) and entries of the last call on `slot`; ttcr_fsm_get_slot_m: row_off[n_rows+1],
 * j[nnz] node indices, v[nnz] values of the grid dtype. */
int ttcr_fsm_raytrace_m(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx,
                        const void* rx, void* tt_out);
int ttcr_fsm_raytrace_rm(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx,
                         const void* rx, void* tt_out);
int ttcr_fsm_slot_m_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz);
int ttcr_fsm_get_slot_m(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* j, void* v);
/* Replaces: the multi-source overloads with m_data, Grid3D::raytrace(Tx[], t0[], Rx[], traveltimes[], [r_data[],] m_data[])
 * (ttcr/Grid3D.h:896-1000), which run the single-source overload per source on host threads -- what ttcrpy reaches with
 * compute_M and several events (src/ttcrpy/rgrid.pyx:1096-1102).  Sources and receivers laid out like ttcr_fsm_raytrace_multi;
 * the fields are solved in batches of n_slots sources (one sweep launch per batch and sweep-iteration instead of one chain of
 * launches per source), the walks follow each batch.  with_rays != 0: the overload with r_data and m_data for every source
 * (rays: ttcr_fsm_rays_size / ttcr_fsm_get_rays).  Results identical to n_src calls of ttcr_fsm_raytrace_m / _rm.
 * ttcr_fsm_multi_m_size / ttcr_fsm_get_multi_m: ONE CSR over all receiver rows of the call (row r = receiver row r). */
int ttcr_fsm_raytrace_multi_m(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                              const void* rx, void* tt_out, int with_rays);
int ttcr_fsm_multi_m_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz);
int ttcr_fsm_get_multi_m(const ttcr_fsm_grid* g, long long* row_off, long long* j, void* v);

/* The M tape: the matrix of ttcr_fsm_raytrace_multi_m (with_rays = 0) kept on the device for M^T w, the gradient of a misfit with
 * respect to node velocity.  No reference counterpart: it derives from the same walk, Grid3Drn::getRaypath(Tx, t0, Rx, m_data, RxNo,
 * tt, threadNo) (ttcr/Grid3Drn.h:1503-1800), whose records are merged on the device instead of being copied to the host.
 * ttcr_fsm_raytrace_multi_tape: sources and receivers laid out like ttcr_fsm_raytrace_multi_m; tt_out as that call gives it (the
 * fields are solved and walked by the same batched path); *tape receives a new tape whose rows are the receiver rows in layout order.
 * Its entries are those of ttcr_fsm_get_multi_m with node indices >= n_nodes dropped, nodes ascending within a row; the values are
 * merged exactly as the host assembly merges them (contributions of one node summed in push order, starting from the first one).
 * 3-D node grids only (TTCR_ERR_UNSUPPORTED otherwise, with compute_M's message).  On a multi-device grid every replica walks its own
 * sources and the parts are put together on the first listed device: the tape is bit-identical to that of a one-device grid.
 * A tape owns its device memory and stream: it stays valid after later calls on the grid, after ttcr_fsm_set_slowness and after
 * ttcr_fsm_destroy of the grid, until ttcr_fsm_tape_free (NULL: no-op).  Calls on one tape from several threads are serialised.
 * ttcr_fsm_tape_size: rows, columns (= n_nodes) and entries.  ttcr_fsm_tape_bytes: device memory the tape holds:
 *   8 (n_rows + 1 + n_nodes + 1) + 2 nnz (4 + elem) + (n_rows + n_nodes) elem   (elem = 4 or 8 bytes, the grid dtype).
 * ttcr_fsm_tape_device: the HIP device the tape lives on.
 * ttcr_fsm_tape_get_csr: host copy, row_off[n_rows + 1], j[nnz] node indices, v[nnz] values of the grid dtype.
 * ttcr_fsm_tape_vjp: grad[n] = sum over the entries of node n, rows ascending, of fl(v * w[row]), summed left to right from +0 in the
 *   grid dtype, without atomics (reproducible to the bit, independent of the device list and of n_slots).  w: n_rows values, grad:
 *   n_nodes values (x fastest), both of the grid dtype; *_on_device != 0: a device pointer on the tape's device, else host memory.
 *   The call returns with grad written.  The tape runs on its own stream: the caller makes sure a device-resident w is complete
 *   before the call (e.g. synchronise the stream that produced it).
 * Argument errors (a NULL tape or pointer) return TTCR_ERR_VALUE before any device call. */
typedef struct ttcr_fsm_tape ttcr_fsm_tape; /* opaque */
int ttcr_fsm_raytrace_multi_tape(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                 const void* rx, void* tt_out, ttcr_fsm_tape** tape);
int ttcr_fsm_tape_size(const ttcr_fsm_tape* t, size_t* n_rows, size_t* n_cols, size_t* nnz);
int ttcr_fsm_tape_bytes(const ttcr_fsm_tape* t, size_t* bytes);
int ttcr_fsm_tape_device(const ttcr_fsm_tape* t, int* device);
int ttcr_fsm_tape_get_csr(const ttcr_fsm_tape* t, long long* row_off, long long* j, void* v);
int ttcr_fsm_tape_vjp(const ttcr_fsm_tape* t, const void* w, int w_on_device, void* grad, int grad_on_device);
int ttcr_fsm_tape_free(ttcr_fsm_tape* t);

/* The field tape: the exact discrete adjoint of the first-order 3-D node solver (adjoint-state gradient).  No reference counterpart.
 * ttcr_fsm_raytrace_multi_adjoint: sources and receivers laid out like ttcr_fsm_raytrace_multi; the same batched solves; tt_out holds the
 * INTERPOLATED receiver traveltimes (Grid3Drn::getTraveltime, ttcr/Grid3Drn.h:794-930), bit-equal to ttcr_fsm_raytrace_multi on a grid with
 * tt_from_rp = 0 whatever this grid's setting (forced for the call, as the l_data overloads force it).  *tape receives a new tape that
 * holds every event's traveltime field (device-to-device copies), one copy of the node slowness, per event the nodes the source
 * initialisation froze with their distances, and per receiver row the interpolation stencil with its weights.
 * 3-D node grids without the WENO stage only (TTCR_ERR_UNSUPPORTED otherwise, the message names the reason).  On a multi-device grid the
 * fields are copied to the first listed device and the adjoint runs there.  A tape owns its device memory and stream: it stays valid
 * after later calls on the grid, after ttcr_fsm_set_slowness and after ttcr_fsm_destroy of the grid, until ttcr_fsm_adjoint_free (NULL:
 * no-op).  If the memory cannot be allocated the call fails with TTCR_ERR_DEVICE and a message that names the byte count.  Calls on one
 * tape from several threads are serialised.
 * ttcr_fsm_adjoint_size: events, receiver rows and nodes.  ttcr_fsm_adjoint_bytes: device memory the tape holds, about
 *   n_events n_nodes (5 elem + 2) bytes (fields, D, seeds, two lam buffers; two byte masks) plus the small lists.
 * ttcr_fsm_adjoint_device: the HIP device the tape lives on.  ttcr_fsm_adjoint_get_field: host copy of the field of one event, n_nodes
 *   values of the grid dtype, x fastest (node (k * nny + j) * nnx + i).
 * ttcr_fsm_adjoint_vjp: grad = d loss / d node slowness (n_nodes values, x fastest) for the cotangents w (one value per receiver row, may
 *   be NULL) and field_cot (n_events * n_nodes values, one per node of every event's field, may be NULL; not both).  With T the field, s
 *   the slowness and F the frozen nodes of an event: a node m outside F couples, along each axis, to the smaller of its two neighbours
 *   (outside the grid: +inf; tie: the lower index) if that is < T[m]; D_m = sum over those axes, x, y, z, of (T[m] - a_axis).  Seeds
 *   g = field_cot + sum over the receiver rows, in row order, of w[row] * weight on the nodes of the row's stencil;
 *   lam[j] = g[j] + sum over the neighbours n of j (x-, x+, y-, y+, z-, z+) that are outside F and couple to j of
 *   fl(fl(lam[n] * (T[n] - T[j])) / D_n);  grad_e[m] = fl(fl(lam[m] * fl(dx * fl(s[m] * dx))) / D_m), or fl(d_m * lam[m]) for m in F;
 *   grad = sum of grad_e over the events, ascending, from +0.  Everything in the grid dtype, without fused multiply-add and without
 *   floating-point atomics: lam is the unique fixed point of the gather formula, so the bits depend neither on the schedule nor on
 *   n_slots nor on the device list.  schedule: 0 the tiled relaxation (tiles staged in LDS), 1 the global Jacobi baseline (bit-equal,
 *   slower); anything else is TTCR_ERR_VALUE.  *passes (may be NULL): relaxation passes launched.  *_on_device != 0: a device pointer on
 *   the tape's device, else host memory.  The call returns with grad written; the tape runs on its own stream: the caller makes sure
 *   device-resident inputs are complete before the call.
 * ttcr_fsm_adjoint_jvp: the forward mode of the same linearisation: for a slowness perturbation ds (n_nodes values, shared
 *   by the events), per event mu = dT/ds . ds with  mu[m] = fl(d_m * ds[m])  for m in F, and otherwise  mu[m] = fl(acc / D_m),
 *   acc = fl(fl(dx * fl(s[m] * dx)) * ds[m]), then for the active axes x, y, z:  acc = fl(acc + fl(mu[u_axis] * fl(T[m] - a_axis)))  (u_axis
 *   the upwind neighbour chosen above, a_axis its T);  dtt[row] = from +0, over the row's stencil entries in stencil order,
 *   acc = fl(acc + fl(weight * mu[node])).  dtt: n_rows values in tape row order; dfields: n_events * n_nodes values (mu of every event);
 *   either may be NULL, not both.  mu is the unique fixed point of a gather from strictly smaller T: the bits depend on no schedule, as
 *   for the vjp; schedule and *passes as there.  The first jvp (or gn) of a tape allocates the stencil in row order, a staging row
 *   and the stamps of its own tiles: 4 (n_rows + 1) + n_entries (8 + elem) + n_rows elem + 4 n_events n_tiles bytes, n_entries the
 *   stencil entries of all rows (at most 8 per row), n_tiles the product over the axes of ceil(nodes / edge), edge = 10 (fp32) or 8
 *   (fp64), which ttcr_fsm_adjoint_bytes reports from then on; TTCR_ERR_DEVICE with the byte count if that fails.
 * ttcr_fsm_adjoint_gn: the Gauss-Newton product out = J^T (row_weight * (J v)) (n_nodes values): the jvp of v, every row multiplied by
 *   row_weight[row] (n_rows values in tape row order; NULL: no weight), the vjp of the result -- with the bits of the two calls composed,
 *   and no host copy in between.  *passes_jvp, *passes_vjp (may be NULL): the passes of the two relaxations.
 * Derivatives with respect to the source points.  The points of a tape are the source points of its events in call order
 *   (tx order); the parameters of a point are (t0, x, y, z), the column order of a ttcrpy source row.  A frozen node m belongs to the
 *   point q(m) that wrote it last, T[m] = t0 + d_m s[m]; c[m][a] = fl(fl(p_a - x_a(m)) / d_m) for a = x, y, z, +0 where d_m = 0 (p the point
 *   as the solver sees it, after the origin shift of a translated grid), computed on the host in the grid dtype when the tape is made.
 *   The map has a kink where a point crosses a cell face or enters the 1e-4 on-node tolerance; the formula is returned there too.
 * ttcr_fsm_adjoint_points: *n_points, and the event of every point (event_of_point: n_points ints, may be NULL).
 * ttcr_fsm_adjoint_jvp_source: n_cols (1 to 4) perturbations at once; dsrc: n_cols x n_points x 4 values.  Per column and event
 *   mu[m] = dsrc[q(m)][0], then for a = x, y, z: acc = fl(acc + fl(fl(s[m] * c[m][a]) * dsrc[q(m)][1 + a]))  for m in F, and otherwise
 *   mu[m] = fl(acc / D_m), acc = +0, then for the active axes x, y, z: acc = fl(acc + fl(mu[u_axis] * fl(T[m] - a_axis)))  -- the jvp above
 *   with ds = +0.  dtt: n_cols x n_rows values (rows as in the jvp); dfields: n_cols x n_events x n_nodes values; either may be NULL, not
 *   both.  n_cols = 1 relaxes one column in the lam buffers; n_cols > 1 relaxes four columns at once, the four values of a node adjacent
 *   in memory (upwind choice, D and differences computed once per node), the columns past n_cols being +0.  Every column has the bits
 *   of the one-column call.  The first jvp_source or vjp_source allocates the frozen entries by point, 4 (n_points + 1) + n_frozen (16 + 3
 *   elem) bytes, and two staging arrays, (16 n_points + 4 n_rows) elem bytes; the first jvp_source what the first jvp allocates; the first
 *   call with n_cols > 1 a work array of 4 n_events n_nodes elem bytes, the first such call with schedule 1 a second one.
 *   ttcr_fsm_adjoint_bytes reports all of it from then on; TTCR_ERR_DEVICE with the byte count if an allocation fails.
 * ttcr_fsm_adjoint_vjp_source: the vjp above and, from the same lam, gsrc (n_points x 4 values):  gsrc[q][0] = from +0, over the frozen
 *   nodes m with q(m) = q in ascending node index, acc = fl(acc + lam[m]);  gsrc[q][1 + a] = the same chain of
 *   fl(lam[m] * fl(s[m] * c[m][a])).  A point all of whose nodes a later point overwrote gets four +0.  grad may be NULL (no slowness
 *   gradient is formed); otherwise it has the bits of ttcr_fsm_adjoint_vjp.  One thread per point, no floating-point atomics.
 * Second-order products (tests/hessian_reference.py restates them).  For a cotangent (w, field_cot) the vjp is a function
 *   of the slowness; its derivative in a direction v, with the cotangent held fixed, is  sum_r w_r (d2 tt_r / ds2) v  (and the same for
 *   the field part): the term a Gauss-Newton product drops.
 * ttcr_fsm_adjoint_hold: the vjp of (w, field_cot) -- grad (may be NULL) has the bits of ttcr_fsm_adjoint_vjp -- whose lam stays on the
 *   tape.  The first hold allocates 2 n_events n_nodes elem bytes (lam and a work array), which ttcr_fsm_adjoint_bytes reports;
 *   TTCR_ERR_DEVICE with the byte count if that fails.  A later hold replaces the held lam.  ttcr_fsm_adjoint_release frees both arrays
 *   (ttcr_fsm_adjoint_bytes falls by the same figure); ttcr_fsm_adjoint_free releases too.
 * ttcr_fsm_adjoint_hvp: out (n_nodes values) for a direction v (n_nodes values).  Per event, mu the jvp field tangent of v, lam the held one:
 *     dD[n]    = over the active axes x, y, z, the first term assigned:  fl(mu[n] - mu[u_axis(n)])                         n not in F
 *     q[j]     = +0, then over the neighbours n that have j as an active upwind neighbour, order x-, x+, y-, y+, z-, z+:
 *                q[j] = fl(q[j] + fl(lam[n] * fl(fl(fl(mu[n] - mu[j]) - fl(fl(fl(T[n] - T[j]) / D_n) * dD[n])) / D_n)))
 *     lam2     = the fixed point of the vjp for the field cotangent q (and no rows)
 *     r[m]     = fl(fl(lam[m] * fl(fl(dx * fl(v[m] * dx)) - fl(fl(fl(dx * fl(s[m] * dx)) / D_m) * dD[m]))) / D_m)           m not in F
 *     out_e[m] = fl(fl(fl(lam2[m] * fl(dx * fl(s[m] * dx))) / D_m) + r[m])  for m not in F,   fl(d_m * lam2[m])  for m in F
 *     out[m]   = the events summed ascending from +0
 *   One tangent and one adjoint relaxation (the kernels of jvp and vjp) and three streaming kernels, on the tape's stream without a host
 *   copy in between; no floating-point atomics; the bits depend on no schedule.  *passes_jvp, *passes_vjp as for ttcr_fsm_adjoint_gn.
 * ttcr_fsm_adjoint_newton: the same with the rows fl(row_weight[row] * (J v)[row]) (row_weight NULL: (J v)[row]) added to the seeds of lam2
 *   exactly as the vjp adds w:  out = J^T W J v + hvp(v)  from ONE adjoint relaxation, the cost of ttcr_fsm_adjoint_gn plus the three
 *   streaming kernels.  The first hvp or newton allocates what the first jvp allocates.
 *   On a cell tape v and out hold n_cells values:  hvp(v) = A^T (node hvp(A v)), likewise newton, A and A^T as for jvp and vjp.
 *   Without a held cotangent both return TTCR_ERR_VALUE (the message says so) before any device call.
 * Block products: the three products above for n_cols >= 1 model vectors per call.  ds, v, grad and out hold n_cols x
 *   n_params values (n_params of ttcr_fsm_adjoint_model), w and dtt n_cols x n_rows values in tape row order, dfields n_cols x n_events x
 *   n_nodes values, column k at k times the length of one column; row_weight holds rw_cols x n_rows values, rw_cols = 0 (none, row_weight
 *   is ignored), 1 (one set shared by the columns) or n_cols (one set per column).  Under schedule 0 the columns are relaxed in groups of
 *   four, the four values of a node adjacent in memory and in LDS: masks, upwind choice, differences, D and the tile stamps are read and
 *   formed once per node, and per column the expressions of the one-column calls are evaluated in their order -- the jvp chain starts from
 *   the own term, the seeds and the gradient from +0, the vjp chain from the seed.  The last group is padded with +0 columns.  Schedule 1
 *   runs the columns one by one through the Jacobi baseline.  Column k of every output has the bits of the one-column call
 *   (ttcr_fsm_adjoint_jvp, _vjp with field_cot NULL, _gn) on column k, whatever n_cols, the position of the column, the schedule, the slots
 *   and the devices of the grid the tape came from.  *passes: the passes of all groups summed.  No floating-point atomics.  On a cell tape
 *   A and A^T are applied column by column with the kernels of the one-column calls.
 *   The first block call allocates the work arrays: the seeds of four columns, 4 n_events n_nodes elem bytes; lam / mu of four columns, as
 *   much again unless a ttcr_fsm_adjoint_jvp_source call with n_cols > 1 allocated that array before; staging for one group, (4 n_params +
 *   8 n_rows) elem bytes and, on a cell tape, 4 n_nodes elem bytes; and what the first jvp allocates if no jvp came before.
 *   ttcr_fsm_adjoint_bytes reports them from then on; TTCR_ERR_DEVICE with the byte count if an allocation fails.
 *   ttcr_fsm_adjoint_block_release frees them (ttcr_fsm_adjoint_bytes falls by the figure the block call added; the next block call
 *   allocates again), ttcr_fsm_adjoint_free too; ttcr_fsm_adjoint_release and a held lam are left alone, and a block call leaves them alone.
 *   Not offered per block: hvp / newton, field cotangents, source-point gradients.
 *   Argument errors -- n_cols < 1, an unknown schedule, a NULL input (ds, w, v) or output (dtt and dfields both NULL, grad, out), rw_cols
 *   not 0, 1 or n_cols, a NULL row_weight with rw_cols != 0, a NULL tape -- return TTCR_ERR_VALUE before any device call.
 * Cell tapes.  ttcr_fsm_raytrace_multi_adjoint_cells: the same call for a 3-D grid with slowness defined for CELLS and
 *   without the WENO stage (a node grid: TTCR_ERR_VALUE, the message names ttcr_fsm_raytrace_multi_adjoint; 2-D and WENO grids:
 *   TTCR_ERR_UNSUPPORTED; ttcr_fsm_raytrace_multi_adjoint itself keeps refusing cell grids).  The solver works on the node slowness
 *   s = A sc, A the averaging of Grid3Drcfs::setSlowness (the mean of the cells that touch a node); the tape holds that s and is the tape
 *   above in everything but its model vector, which has n_cells = ncx ncy ncz values, cell (ck * ncy + cj) * ncx + ci, x fastest -- the
 *   order ttcr_fsm_set_slowness takes.  On such a tape grad of ttcr_fsm_adjoint_vjp and ttcr_fsm_adjoint_vjp_source, ds of
 *   ttcr_fsm_adjoint_jvp, v and out of ttcr_fsm_adjoint_gn hold n_cells values:  jvp(ds) = node jvp(A ds), A ds with the arithmetic and
 *   summation order of ttcr_fsm_set_slowness (its kernel);  vjp = A^T (node vjp), with  (A^T g)[c] = the eight products fl(f(n) * g[n]) over
 *   the corner nodes n = (ci + a, cj + b, ck + d) of the cell, f(n) = 1 / (number of cells that touch n), added left to right from the
 *   first product, a innermost, d outermost, lower index first, in the grid dtype, without fused multiply-add; one thread per cell, no
 *   atomics;  gn(v) = A^T J^T W J A v, on the tape's stream without a host copy in between.  field_cot, dfields, the field of
 *   ttcr_fsm_adjoint_get_field and the third output of ttcr_fsm_adjoint_size stay n_nodes; the source-point calls are unchanged.  A cell
 *   tape holds n_cells elem bytes more (a staging vector for host arrays), which ttcr_fsm_adjoint_bytes reports.
 * ttcr_fsm_adjoint_model: *cells = 1 for a cell tape, 0 for a node tape; *n_params the length of its model vector (n_cells or n_nodes;
 *   mx my mz on a model tape, for which *cells = 0); *n_nodes the nodes of a field.
 * Model tapes (tests/model_reference.py restates every expression).  ttcr_fsm_model_raytrace_multi_adjoint: the call of
 *   ttcr_fsm_raytrace_multi_adjoint for a 3-D node grid, with model_shape = (mx, my, mz), 1 <= m_d <= n_d: the model vector of the tape
 *   holds the slowness at the nodes of a coarse grid, uniform per axis and spanning the fine grid exactly, x fastest; m_d = 1 means
 *   constant along that axis ((1, 1, mz): a layered model).  A cell grid or a shape outside the range: TTCR_ERR_VALUE; 2-D and WENO
 *   grids: TTCR_ERR_UNSUPPORTED; all before any device call.  The node vector is P times the model vector, P the trilinear
 *   prolongation.  Per axis and fine index i, in 64-bit integers: q = i (m - 1), I = q div (n - 1), r = q mod (n - 1), the last fine
 *   node taking I = m - 2, r = n - 1; wl = T((n - 1 - r) / (n - 1)), wh = T(r / (n - 1)), each quotient in double, rounded to the grid
 *   dtype once; m = 1: I = 0, wl = 1, no upper term.  A term whose weight is exactly 0 is left out of every sum, so m = n gives the
 *   identity bit for bit.  No fused multiply-add.  (P v)(i, j, k): lerp_x over the four x-pairs of the eight surrounding model nodes,
 *   lerp_y over the two pairs of results, lerp_z; lerp(a, b) = fl(wl a) + fl(wh b), lower index first.  P^T g in three stages, z first:
 *   a[i, j, K] = the sum over the fine k, ascending, from the first term, of fl(w g[i, j, k]) for the k with I_z(k) == K (w = wl) or
 *   I_z(k) + 1 == K (w = wh); the same over j, then over i.  One thread per output element, no atomics.  On such a tape
 *   vjp = P^T (node vjp), jvp(v) = node jvp(P v), gn(v) = P^T J^T B J P v, hold / hvp / newton and the block, joint, receiver-joint and
 *   double-difference products compose the same way; the tape linearises at the slowness that was solved, which need not be P of
 *   anything.  Smoothing (ttcr_fsm_normal_smooth, the solves) acts on the model grid with spacing h_d = dx (n_d - 1) / (m_d - 1) per
 *   axis; an axis with m_d < 3 is left out of R and has to have weight 0 (TTCR_ERR_VALUE otherwise).  A model tape holds the staged
 *   model vector, the axis tables and the two intermediates of P^T (nx ny mz and nx my mz values) more than a node tape;
 *   ttcr_fsm_adjoint_bytes counts them.
 * ttcr_fsm_model_shape: *is_model = 1 and shape = (mx, my, mz) for a model tape, 0 and zeros otherwise.
 * ttcr_fsm_model_tape_prolong / ttcr_fsm_model_tape_restrict: out = P v (n_nodes values) / out = P^T g (mx my mz values) with the
 *   tape's tables on the tape's stream; host or device pointers as for the products.  A tape without a model grid: TTCR_ERR_VALUE.
 * ttcr_fsm_model_prolong / ttcr_fsm_model_restrict: the same maps on a grid, before any tape exists, for any model_shape the tape entry
 *   would take (the same refusals); device pointers are on the grid's device.  ttcr_fsm_model_device: that device (the first one
 *   of a grid on a device list).
 * Argument errors (a NULL tape or pointer, w and field_cot both NULL, dtt and dfields both NULL, n_cols outside 1 to 4, an unknown
 * schedule) return TTCR_ERR_VALUE before any device call. */
typedef struct ttcr_fsm_adjoint ttcr_fsm_adjoint; /* opaque */
int ttcr_fsm_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                    const void* rx, void* tt_out, ttcr_fsm_adjoint** tape);
int ttcr_fsm_raytrace_multi_adjoint_cells(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                          const void* rx, void* tt_out, ttcr_fsm_adjoint** tape);
int ttcr_fsm_adjoint_model(const ttcr_fsm_adjoint* t, int* cells, size_t* n_params, size_t* n_nodes);
int ttcr_fsm_model_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                          const void* rx, void* tt_out, ttcr_fsm_adjoint** tape, const int model_shape[3]);
int ttcr_fsm_model_shape(const ttcr_fsm_adjoint* t, int* is_model, int* shape);
int ttcr_fsm_model_tape_prolong(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device);
int ttcr_fsm_model_tape_restrict(const ttcr_fsm_adjoint* t, const void* g, int g_on_device, void* out, int out_on_device);
int ttcr_fsm_model_device(const ttcr_fsm_grid* g, int* device);
int ttcr_fsm_model_prolong(ttcr_fsm_grid* g, const int model_shape[3], const void* v, int v_on_device, void* out, int out_on_device);
int ttcr_fsm_model_restrict(ttcr_fsm_grid* g, const int model_shape[3], const void* gr, int g_on_device, void* out, int out_on_device);
int ttcr_fsm_adjoint_size(const ttcr_fsm_adjoint* t, size_t* n_events, size_t* n_rows, size_t* n_nodes);
int ttcr_fsm_adjoint_bytes(const ttcr_fsm_adjoint* t, size_t* bytes);
int ttcr_fsm_adjoint_device(const ttcr_fsm_adjoint* t, int* device);
int ttcr_fsm_adjoint_get_field(const ttcr_fsm_adjoint* t, size_t event, void* out);
int ttcr_fsm_adjoint_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                         int grad_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, void* dtt, int dtt_on_device, void* dfields,
                         int df_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device, void* out,
                        int out_on_device, int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_adjoint_points(const ttcr_fsm_adjoint* t, size_t* n_points, int* event_of_point);
int ttcr_fsm_adjoint_jvp_source(const ttcr_fsm_adjoint* t, const void* dsrc, int dsrc_on_device, int n_cols, void* dtt, int dtt_on_device,
                                void* dfields, int df_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_vjp_source(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                                int grad_on_device, void* gsrc, int gsrc_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_hold(ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                          int grad_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_release(ttcr_fsm_adjoint* t);
int ttcr_fsm_adjoint_hvp(ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device, int schedule, int* passes_jvp,
                         int* passes_vjp);
int ttcr_fsm_adjoint_newton(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device, void* out,
                            int out_on_device, int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_adjoint_jvp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* ds, int ds_on_device, void* dtt, int dtt_on_device,
                               void* dfields, int df_on_device, int schedule, int* passes);
int ttcr_fsm_adjoint_vjp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* w, int w_on_device, void* grad, int grad_on_device,
                               int schedule, int* passes);
int ttcr_fsm_adjoint_gn_block(const ttcr_fsm_adjoint* t, int n_cols, const void* v, int v_on_device, const void* row_weight,
                              int rw_cols, int rw_on_device, void* out, int out_on_device, int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_adjoint_block_release(ttcr_fsm_adjoint* t);
int ttcr_fsm_adjoint_free(ttcr_fsm_adjoint* t);

/* The normal equations of a field tape: the step of a damped, smoothed least-squares inversion,
 *     (H + smooth R + damp I) x = rhs,   H = J^T W J of ttcr_fsm_adjoint_gn or the Newton product of ttcr_fsm_adjoint_newton,
 * solved by conjugate gradients on the tape's stream.  No reference counterpart.  Model vectors hold n_params values (n_params of
 * ttcr_fsm_adjoint_model) in the tape's order, x fastest: nx x ny x nz nodes, or the (nx - 1) x (ny - 1) x (nz - 1) cells of a cell
 * tape.  Every value is one fixed expression in the grid dtype T, each operation rounded, no fused multiply-add, no floating-point
 * atomics; tests/normal_reference.py restates all of it.  An `_on_device` pointer is used in place, a host pointer is staged.
 * ttcr_fsm_normal_smooth: out = R v = sum_d weights[d] K_d^T (K_d v), d = x, y, z; K_d the order-2 operator of Grid3d.compute_K
 *   along axis d (second differences of spacing dx, the centred stencil shifted inwards on the two end rows).  Along an axis of length
 *   n, with c(r) = clip(r, 1, n - 2) and ih2 = T(1 / (dx dx)) (the quotient in double, then rounded):
 *     y[r] = fl(fl(fl(v[c - 1] + v[c + 1]) - fl(2 v[c])) * ih2)
 *     z[i] = the sum, over the rows r that touch i in ascending r, from the first term, of fl(coef * y[r]): row 0 if i <= 2 (coef ih2,
 *            -2 ih2, ih2 for i = 0, 1, 2), rows r in {i - 1, i, i + 1} with 1 <= r <= n - 2 (ih2, -2 ih2, ih2 for r = i + 1, i, i - 1), row
 *            n - 1 if i >= n - 3 (ih2, -2 ih2, ih2 for i = n - 3, n - 2, n - 1)
 *     out[m] = fl(fl(fl(a_x z_x) + fl(a_y z_y)) + fl(a_z z_z)),  a_d = T(weights[d])
 *   One kernel: a tile of v (ttcr_fsm_normal_tile_edge(dtype)^3 parameters, 16 for fp32 and 12 for fp64) with a two-node halo in LDS, y
 *   recomputed.  v and out are different arrays.  An axis with fewer than 3 parameters: TTCR_ERR_VALUE.
 * ttcr_fsm_normal_dot: *result = <a, b> in fp64 with a fixed summation order.  e[i] = double(a[i]) * double(b[i]) (exact for fp32,
 *   rounded for fp64), +0 past the end.  Chunk c = elements [1024 c, 1024 c + 1024), one workgroup of 256 threads: thread t forms
 *   ((e[t] + e[t + 256]) + e[t + 512]) + e[t + 768], then for stride = 128, 64, ..., 1: s[t] += s[t + stride] for t < stride.  One
 *   workgroup closes the sum: thread t adds the chunk partials t, t + 256, ... ascending from +0, then the same halving.
 * ttcr_fsm_normal_solve: A p = fl(fl(H p + fl(T(smooth) * (R p))) + fl(T(damp) * p)), the smooth term not evaluated for smooth == 0, the
 *   damp term not for damp == 0; H p has the bits of ttcr_fsm_adjoint_gn (newton = 1: ttcr_fsm_adjoint_newton, which needs a held
 *   cotangent; TTCR_ERR_VALUE with the message of that entry without one).  Vectors in T, scalars in fp64, inner products as above:
 *     x = x0 (NULL: +0);  r = rhs (x0 given: fl(rhs - A x0));  p = r;  rho = <r, r>;  rho0 = <rhs, rhs>
 *     for k = 1 .. maxiter:  if rho <= rtol rtol rho0: status 0, stop
 *        q = A p;  pq = <p, q>;  if not (pq > 0) or not finite: status 2, stop (x is the iterate so far)
 *        aT = T(rho / pq);  x = fl(x + fl(aT p));  r = fl(r - fl(aT q))
 *        rho_new = <r, r>;  bT = T(rho_new / rho);  p = fl(r + fl(bT p));  rho = rho_new
 *     status 1 if the loop ends without meeting the test
 *   Per iteration: the tape's product, kernel 1 (the smoothing gather of p -- the expression of ttcr_fsm_normal_smooth, read from global
 *   memory because a workgroup owns a chunk of the flat vector here, not a tile --, q and the chunk partials of <p, q>), the finishing
 *   reduction (pq, aT, the flag "pq > 0 and finite"), kernel 2 (x, r and the chunk partials of <r, r>), the finishing reduction (rho,
 *   bT), kernel 3 (p) -- the scalars are formed on the device and read by the update kernels from device memory, which do nothing once
 *   the flag is down -- and ONE host read of (rho, pq) for the stop test and the history.
 *   Outputs: x (n_params values); *status; *iterations, the completed updates of x; rho: maxiter + 2 doubles, of which 2 + *iterations
 *   are written -- rho0, <r, r> of the starting residual, then rho after every completed iteration; pq: maxiter doubles, one per iteration
 *   that evaluated it (*iterations of them, one more after status 2); passes (may be NULL): 2 (maxiter + 1) ints, the (jvp, vjp)
 *   relaxation passes of A x0 (0, 0 without x0) and then of every such iteration.  row_weight: n_rows values in tape row order or NULL.
 *   The first smooth, dot or solve of a tape allocates the work arrays: x, r, p, q and the product output (n_params elem bytes each),
 *   one double per chunk and 48 bytes of scalars; ttcr_fsm_adjoint_bytes reports them from then on; TTCR_ERR_DEVICE with the byte count
 *   if an allocation fails.  ttcr_fsm_normal_release frees them (ttcr_fsm_adjoint_bytes falls by the same figure; the next call
 *   allocates again), ttcr_fsm_adjoint_free too.
 *   Argument errors -- smooth, damp or rtol negative or not finite, maxiter < 1, newton not 0 or 1, weights that are NULL, negative or
 *   not finite, an unknown schedule, a NULL rhs, x, status, iterations, rho or pq, a NULL tape, smooth > 0 on a tape with an axis of
 *   fewer than 3 parameters -- return TTCR_ERR_VALUE with a message that names the argument, in this order, before any device call.
 * Measured (one MI355X, fp32, 441 receivers per event, 10 iterations, smooth and damp > 0; scripts/normal_solve_time.py,
 * profiles/normal_solve/; medians of 5): 128^3 x 16 events, ttcr_fsm_normal_solve 403.5 ms, the ten ttcr_fsm_adjoint_gn calls alone
 * 403.3 / 402.8 ms (before / after); 256^3 x 8 events, 2049.2 ms against 2049.0 / 2048.0 ms.  The differences are below the spread of
 * the run (1 to 3 ms): the cost the solver adds per iteration is not resolved, it is below 0.3 ms.  The same loop with torch operations
 * around the Gauss-Newton product: 405.2 and 2056.5 ms. */
int ttcr_fsm_normal_tile_edge(int dtype);
int ttcr_fsm_normal_smooth(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const double* weights, void* out, int out_on_device);
int ttcr_fsm_normal_dot(ttcr_fsm_adjoint* t, const void* a, int a_on_device, const void* b, int b_on_device, double* result);
int ttcr_fsm_normal_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* row_weight, int rw_on_device, double smooth,
                          const double* smooth_weights, double damp, const void* x0, int x0_on_device, int maxiter, double rtol,
                          int newton, int schedule, void* x, int x_on_device, int* status, int* iterations, double* rho, double* pq,
                          int* passes);
int ttcr_fsm_normal_release(ttcr_fsm_adjoint* t);

/* The joint hypocentre-velocity system of a field tape: the slowness block and the source block of the same
 * linearisation in one product and one solve.  A joint vector has n_joint = n_params + 4 n_points elements: the model vector, then
 * (t0, x, y, z) of every source point in call order (ttcr_fsm_adjoint_points); the entries take and return its two blocks as two
 * arrays.  All arithmetic in the grid dtype T, every operation rounded on its own; tests/joint_reference.py restates all of it.
 * ttcr_fsm_joint_jvp: dtt (n_rows, tape row order) and / or dfields (n_events x n_nodes) = the tangent of (ds, dsrc) from ONE
 *   relaxation: a frozen node m holds fl(fl(d_m ds[m]) + sigma[m]), sigma the frozen-node expression of ttcr_fsm_adjoint_jvp_source for
 *   dsrc of the point that wrote m last, and is never rewritten; every other node obeys ttcr_fsm_adjoint_jvp's expression.  The values
 *   are those of ttcr_fsm_adjoint_jvp for dsrc == 0 and of ttcr_fsm_adjoint_jvp_source for ds == 0 (the sign of a zero may differ).
 * ttcr_fsm_joint_gn: (out, out_src) = (g_s, fl(c * g_e')) with (g_s, g_e') the bits of ttcr_fsm_adjoint_vjp_source applied to
 *   fl(row_weight * dtt), dtt the joint tangent of (v, fl(c * v_src)); c = source_scale, 4 n_points host doubles >= 0 rounded to T, or
 *   NULL: no scaling and no multiplication.  A scale of 0 fixes that parameter.
 * ttcr_fsm_joint_solve: conjugate gradients from zero on
 *       [ Hss + smooth R + damp I    Hse C             ] [x_s]   [ rhs       ]
 *       [ C Hes                      C Hee C + diag(d) ] [z_e] = [ C rhs_src ],        x_src = fl(c * z_e),
 *   d = source_damp (4 n_points host doubles >= 0 or NULL), which acts on the scaled unknown z_e; rhs_src is handed over unscaled, as
 *   ttcr_fsm_adjoint_vjp_source returns it.  A p: the slowness block is ttcr_fsm_normal_solve's expression, the source block
 *   fl(g_e + fl(T(d) * p_e)); a term whose factor is 0 everywhere is not evaluated.  Inner products, recurrence, scalars, statuses, the
 *   one host read per iteration and the outputs status, iterations, rho (maxiter + 2), pq (maxiter) are ttcr_fsm_normal_solve's, the
 *   inner products over the flat joint vector in chunks of 1024 with the block seam wherever it falls; passes (may be NULL): 2 maxiter
 *   ints.  With source_scale all zeros x_src is zero and x equals ttcr_fsm_normal_solve's element for element.  No x0, no Newton product.
 *   The first solve allocates work arrays of its own -- five joint vectors, three source blocks, one double per chunk of 1024 joint
 *   elements, 48 bytes of scalars -- which ttcr_fsm_adjoint_bytes reports; TTCR_ERR_DEVICE with the byte count if that fails;
 *   ttcr_fsm_joint_release (and ttcr_fsm_adjoint_free) return them.  The arrays of ttcr_fsm_normal_* are not touched.
 * Argument errors (a NULL array or tape, smooth, damp, rtol, a source_scale or source_damp value negative or not finite, maxiter < 1, an
 * unknown schedule, smooth > 0 with an axis of fewer than 3 parameters) return TTCR_ERR_VALUE naming the argument before any device call.
 * Kernels: one seed kernel (a thread per frozen entry), the tangent's tiled and global-Jacobi relaxations compiled with the frozen nodes
 * left alone, one element-wise scale kernel, kernel 1 of the solver over n_joint elements; everything else is the existing kernels.  No
 * floating-point atomics.  Measurements: DESIGN.md 6j (scripts/joint_time.py, profiles/joint_solve/). */
int ttcr_fsm_joint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* dsrc, int dsrc_on_device, void* dtt,
                       int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes);
int ttcr_fsm_joint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_src, int vs_on_device, const void* row_weight,
                      int rw_on_device, const double* source_scale, void* out, int out_on_device, void* out_src, int os_on_device,
                      int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_joint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_src, int rs_on_device,
                         const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                         const double* source_damp, const double* source_scale, int maxiter, double rtol, int schedule, void* x,
                         int x_on_device, void* x_src, int xs_on_device, int* status, int* iterations, double* rho, double* pq, int* passes);
int ttcr_fsm_joint_release(ttcr_fsm_adjoint* t);

/* Derivatives of the returned traveltimes with respect to the RECEIVER points of a field tape, and the joint system with the receiver
 * block in the place of the source block -- what a reciprocal layout needs: solve from the stations, read the traveltimes
 * at the hypocentres, which are then the receivers of the call.  For a tape row r the receiver p is taken as the solver sees it (after the
 * origin shift of a translated grid); G[r][a] = d tt[r] / d p_a (a = x, y, z) is the derivative of the trilinear interpolation exactly as
 * the solver evaluates it, with the cell and the on-plane flags held fixed: +0 on an axis the point lies on (within 1e-8), otherwise
 * fl(I_a / dx), I_a the solver's nested interpolation over the remaining axes (z, then y, then x) of the differences
 * fl(T[upper node] - T[lower node]) along a; a clamped upper node gives +0.  All arithmetic in the grid dtype, every operation rounded
 * on its own; tests/receiver_reference.py restates all of it.
 * Receiver points: the tape has n_rcv_points points with parameters (t0, x, y, z) each and a map from rows to points; one point per row
 * by default.  ttcr_fsm_rcv_points: with set_point_of_row != NULL replaces the map (n_rows ints in tape row order, values in
 * 0 .. set_n_points - 1; rows that share a point must have bit-equal receiver coordinates, else TTCR_ERR_VALUE naming the first offending
 * pair of tape rows, which differing_rows (2 ints, may be NULL) receives; at most 2^29 points; a point may have no rows) and frees what
 * the receiver calls hold on the device; then, either way, returns the
 * number of points in *n_points and the map in point_of_row (each may be NULL).
 * ttcr_fsm_rcv_eval: for n_pts queries, pts (3 n_pts values of the grid dtype, user coordinates) read in the field of event
 *   event_of_pt[i] (host ints): tt (n_pts, may be NULL) with the bits of ttcr_fsm_interp on that field, grad (3 n_pts, may be NULL) = G.
 *   No solve, no relaxation.  Node indices are clamped, so a point outside the grid reads the nearest cell.  Events, host points and
 *   host results are staged in one buffer of the tape (7 n_pts values and n_pts ints) that grows to the largest call, is reported by
 *   ttcr_fsm_adjoint_bytes and returned by ttcr_fsm_rcv_release: a loop of calls allocates once.  pts == NULL: the tape's own
 *   rows (n_pts and event_of_pt ignored; n_rows values, tape row order), evaluated once and kept on the tape.
 * ttcr_fsm_rcv_jvp: dtt[r] = acc, acc = drcv[q][0], then for a = x, y, z acc = fl(acc + fl(G[r][a] * drcv[q][1 + a])), q the point
 *   of row r.  ttcr_fsm_rcv_vjp: grcv[q][0] = the sum of w[r], grcv[q][1 + a] the sum of fl(w[r] * G[r][a]) over the rows of q in
 *   ascending tape row order from +0 (one thread per value; a point without rows gets +0).
 * ttcr_fsm_rjoint_jvp: dtt[r] = fl(jvp(ds)[r] + jvp_rcv(drcv)[r]); dfields is ttcr_fsm_adjoint_jvp's.
 * ttcr_fsm_rjoint_gn and ttcr_fsm_rjoint_solve: ttcr_fsm_joint_gn and ttcr_fsm_joint_solve with the receiver block (4 n_rcv_points values)
 *   in the place of the source block: out has the bits of ttcr_fsm_adjoint_vjp, out_rcv = fl(c * grcv); the system, its scaling (rcv_scale),
 *   the damping of the scaled unknown (rcv_damp), inner products, recurrence, statuses and outputs are those of ttcr_fsm_joint_solve with
 *   n_joint = n_params + 4 n_rcv_points.  With rcv_scale all zeros x_rcv is zero and x equals ttcr_fsm_normal_solve's element for element.
 * The first receiver call uploads the receivers and the map, evaluates G of the rows and allocates its staging arrays (3 n_rows + 3
 * n_rows + n_rows + 16 n_rcv_points values, 3 n_rows + n_rcv_points + 1 ints); the first rjoint_solve allocates work arrays of its own,
 * as ttcr_fsm_joint_solve does for n_joint; ttcr_fsm_adjoint_bytes reports both, TTCR_ERR_DEVICE with the byte count if an allocation
 * fails, ttcr_fsm_rcv_release (and ttcr_fsm_adjoint_free) return both.  No other entry's memory changes.
 * Argument errors return TTCR_ERR_VALUE naming the argument before any device call.  Kernels: one evaluation kernel (a thread per
 * query), one row kernel (a thread per row), one gradient kernel (a thread per point and parameter); everything else is the existing
 * kernels.  No floating-point atomics.  Not covered: 2-D, WENO, tt_from_rp = 1, second derivatives. */
int ttcr_fsm_rcv_eval(const ttcr_fsm_adjoint* t, size_t n_pts, const void* pts, int pts_on_device, const int* event_of_pt, void* tt,
                              int tt_on_device, void* grad, int grad_on_device);
int ttcr_fsm_rcv_points(ttcr_fsm_adjoint* t, const int* set_point_of_row, size_t set_n_points, size_t* n_points, int* point_of_row,
                        int* differing_rows);
int ttcr_fsm_rcv_jvp(const ttcr_fsm_adjoint* t, const void* drcv, int drcv_on_device, void* dtt, int dtt_on_device);
int ttcr_fsm_rcv_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, void* grcv, int grcv_on_device);
int ttcr_fsm_rjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* drcv, int drcv_on_device, void* dtt,
                        int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes);
int ttcr_fsm_rjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_rcv, int vr_on_device, const void* row_weight,
                       int rw_on_device, const double* rcv_scale, void* out, int out_on_device, void* out_rcv, int or_on_device,
                       int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_rjoint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_rcv, int rr_on_device,
                          const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                          const double* rcv_damp, const double* rcv_scale, int maxiter, double rtol, int schedule, void* x,
                          int x_on_device, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq, int* passes);
int ttcr_fsm_rcv_release(ttcr_fsm_adjoint* t);

/* Grid-search hypocentre location on the fields of a field tape (no reference equivalent): for the reciprocal layout, in
 * which the tape holds the traveltime from every station (a field) to every node, the node with the smallest weighted,
 * origin-time-corrected misfit of every hypocentre's picks -- the start a Geiger relocation (ttcr_fsm_rcv_eval) needs.  The fields are
 * read once; nothing is solved or relaxed.  Node or cell tapes alike (the fields hold n_nodes values either way).
 * Definition, in float64 whatever the tape's dtype, every operation rounded on its own (no fused multiply-add), sums from +0 in ascending
 * pick order; tests/locate_reference.py restates it.  For hypocentre q with picks k (field f_k, time t_k, weight w_k) and node m:
 *   sw = sum_k w_k      r_k = fl(t_k - double(T[f_k][m]))      a = sum_k fl(w_k * r_k)      t0 = fl(a / sw)
 *   d_k = fl(r_k - t0)  phi = sum_k fl(w_k * fl(d_k * d_k))
 * node_out[q] is the node of the box with the smallest phi, the lowest node index among equal ones (== on doubles); a NaN phi never wins;
 * t0_out[q] and misfit_out[q] are t0 and phi there.  A hypocentre with sw == 0 (no picks, or all weights zero) or with every phi NaN gets
 * node -1, t0 +0 and misfit +0.  The minimum over (phi, node) is associative and commutative: no launch shape shows in the bits.
 * ttcr_fsm_loc_grid: hypo_off (n_hypo + 1, from 0, ascending) are the picks of every hypocentre in pick_field / pick_time / pick_weight
 *   (host arrays; pick_weight == NULL: all ones; a field may occur several times in one hypocentre); box (may be NULL: the whole grid) =
 *   i0, i1, j0, j1, k0, k1, half-open node ranges; node_out holds indices of the whole grid ((k nny + j) nnx + i).  volume_out (may be
 *   NULL): phi of every box node, n_hypo x (box nodes, x fastest within the box) doubles, rows with sw == 0 all +0, on the host or
 *   (volume_on_device != 0) on the tape's device.  At most 2^22 hypocentres and 2^31 - 1 picks per call.
 * ttcr_fsm_loc_geometry: the node counts nn[3], the spacing and the origin in the user's coordinates -- node i of an axis lies at
 *   origin + i dx, as ttcr_fsm_rcv_eval expects a point (translated grids included).
 * ttcr_fsm_loc_shape: the nodes of a node tile and the hypocentres of a chunk of the search kernel on this tape, and whether the tile's
 *   field values are staged in LDS (tests place their sizes around both).
 * The uploaded picks, the partial minima (one per workgroup along the node tiles and hypocentre) and a host volume live in buffers of the
 * tape that grow to the largest call; ttcr_fsm_adjoint_bytes reports them, TTCR_ERR_DEVICE with the byte count if an allocation fails,
 * ttcr_fsm_loc_release (and ttcr_fsm_adjoint_free) return them.  No other entry's memory changes.
 * Argument errors return TTCR_ERR_VALUE naming the argument before any device call: null hypo_off or outputs, offsets that do not start
 * at 0 or are not ascending, a time that is not finite, a weight that is negative or not finite, a null tape, a field out of range, a box
 * outside the grid or empty.  Two kernels: the search (a workgroup per set of node tiles and chunk of hypocentres, partial minima) and
 * the finish (a thread per hypocentre).  No atomics.  Not covered: L1 / EDT misfits, coarse-to-fine search, differential times, 2-D. */
int ttcr_fsm_loc_geometry(const ttcr_fsm_adjoint* t, int* nn, double* dx, double* origin);
int ttcr_fsm_loc_shape(const ttcr_fsm_adjoint* t, int* node_tile, int* hypo_chunk, int* staged);
int ttcr_fsm_loc_grid(const ttcr_fsm_adjoint* t, size_t n_hypo, const long long* hypo_off, const int* pick_field, const double* pick_time,
                      const double* pick_weight, const int* box, long long* node_out, double* t0_out, double* misfit_out,
                      void* volume_out, int volume_on_device);
int ttcr_fsm_loc_release(ttcr_fsm_adjoint* t);

/* Double-difference rows of a field tape (no reference equivalent): the data operator of the Gauss-Newton / Newton products
 * and of the three solves as B = diag(row_weight) + Q^T diag(pair_weight) Q instead of the diagonal alone.  Row p of Q holds +1 at tape
 * row a_p and -1 at tape row b_p: the difference of two rows, e.g. the arrival-time difference of two neighbouring events at one station
 * (hypoDD / tomoDD).  Pairs may join rows of any two events of the tape, may repeat, and a row may be in no pair; the default is no pairs.
 * Definition in the tape's dtype, every operation rounded on its own (no fused multiply-add), no atomics; tests/dd_reference.py restates it.
 * The entries of row r are the pairs p with a_p == r (sign +) or b_p == r (sign -), in ascending p.
 *   Q x:    d[p] = fl(x[a_p] - x[b_p])
 *   Q^T y:  out[r] = a chain from +0 over the entries of r, acc = fl(acc + y[p]) or fl(acc - y[p])
 *   B x:    u[p] = fl(pw[p] * d[p]);  out[r] = a chain from fl(rw[r] * x[r]) (row_weight == NULL: from x[r]) over the entries of r,
 *           acc = fl(acc + u[p]) or fl(acc - u[p])
 * A product with pair_weight has the bits of the product it extends with its fl(row_weight * dtt) step replaced by B dtt; everything
 * before and after that step is unchanged.  With no pairs and an empty pair_weight the bits are those of the call without pair_weight.
 * A vector that is constant over the rows is in the null space of Q: pure double-difference data (row_weight all zero) leave the common
 * origin-time shift of the joint systems undetermined, which is what source_damp / rcv_damp are for.
 * ttcr_fsm_dd_pairs: set_row_a / set_row_b (both NULL: query only) replace the pair list, set_n_pairs pairs in tape rows; the CSR by row
 *   is built on the host and what earlier pair calls hold on the device is freed.  Refused with TTCR_ERR_VALUE, *bad_pair (may be NULL; -1
 *   otherwise) receiving the first offending pair: a == b, a row outside 0 .. n_rows - 1; more than 2^30 - 1 pairs.  n_pairs, row_a, row_b
 *   (may be NULL) receive the list as it stands.
 * ttcr_fsm_dd_apply: mode 0: out (n_pairs) = Q x, x n_rows values; mode 1: out (n_rows) = Q^T x, x n_pairs values; mode 2: out (n_rows) =
 *   B x with row_weight (n_rows, may be NULL) and pair_weight (n_pairs; NULL: ones, u = d without a multiplication).  x and out are
 *   different arrays.
 * ttcr_fsm_dd_gn: system 0: ttcr_fsm_adjoint_gn (newton != 0: ttcr_fsm_adjoint_newton; v_b, b_scale, out_b unused); system 1:
 *   ttcr_fsm_joint_gn; system 2: ttcr_fsm_rjoint_gn -- with pair_weight (n_pairs values, host or device, not NULL), otherwise the
 *   arguments, checks and results of that entry.
 * ttcr_fsm_dd_solve: system 0: ttcr_fsm_normal_solve (rhs_b, b_damp, b_scale, x_b unused); 1: ttcr_fsm_joint_solve; 2:
 *   ttcr_fsm_rjoint_solve (x0 and newton: system 0 only) -- the same conjugate gradients on the products above.
 * Work arrays: the CSR, a, b, one pair array, one staging array for a host pair_weight and one row array, allocated by the first call that
 *   uses pairs, counted by ttcr_fsm_adjoint_bytes, TTCR_ERR_DEVICE with the byte count if that fails; ttcr_fsm_dd_release (and
 *   ttcr_fsm_adjoint_free) return them, the pairs stay as set.  Before ttcr_fsm_dd_pairs no entry's memory changes.
 * Argument errors return TTCR_ERR_VALUE naming the argument before any device call: a bad mode / system / newton, null arrays, a null
 *   tape, no pairs set, a host pair_weight that is negative or not finite, and the errors of the entry a call extends.  Two kernels (one
 *   thread per pair, one thread per row) on the tape's stream.  Not covered: pairs in the block products, differential times in
 *   ttcr_fsm_loc_grid, a relocation-only system, 2-D. */
int ttcr_fsm_dd_pairs(ttcr_fsm_adjoint* t, const int* set_row_a, const int* set_row_b, size_t set_n_pairs, size_t* n_pairs, int* row_a,
                      int* row_b, long long* bad_pair);
int ttcr_fsm_dd_apply(const ttcr_fsm_adjoint* t, int mode, const void* x, int x_on_device, const void* row_weight, int rw_on_device,
                      const void* pair_weight, int pw_on_device, void* out, int out_on_device);
int ttcr_fsm_dd_gn(const ttcr_fsm_adjoint* t, int system, int newton, const void* v, int v_on_device, const void* v_b, int vb_on_device,
                   const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device, const double* b_scale, void* out,
                   int out_on_device, void* out_b, int ob_on_device, int schedule, int* passes_jvp, int* passes_vjp);
int ttcr_fsm_dd_solve(ttcr_fsm_adjoint* t, int system, const void* rhs, int rhs_on_device, const void* rhs_b, int rb_on_device,
                      const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device, double smooth,
                      const double* smooth_weights, double damp, const double* b_damp, const double* b_scale, const void* x0,
                      int x0_on_device, int maxiter, double rtol, int newton, int schedule, void* x, int x_on_device, void* x_b,
                      int xb_on_device, int* status, int* iterations, double* rho, double* pq, int* passes);
int ttcr_fsm_dd_release(ttcr_fsm_adjoint* t);

/* Moving the receiver points of a field tape without a solve, and the relocation-only system (no reference equivalent) --
 * what a relocation loop on a fixed model needs in the reciprocal layout: the fields of the stations stay, the hypocentres (the receiver
 * points of the tape) move, and the step that moves them is the receiver block alone.  tests/relocation_reference.py restates both.
 * ttcr_fsm_reloc_move: pts holds 3 n_rcv_points values of the grid dtype (user coordinates, host or the tape's device); every row of
 *   receiver point q gets the receiver pts[q].  Per row, one thread: the origin of a translated grid is subtracted as the raytrace entry
 *   subtracts it, then the row's interpolation stencil, its traveltime (the bits of ttcr_fsm_interp on the event's field) and G are
 *   evaluated.  The stencil entries in row order (the forward mode's list) are written by that kernel at offsets the host formed; the
 *   adjoint's seed list is that list stably sorted by (event * n_nodes + node) on the device (radix sort) -- the order the host builds for
 *   a new tape.  tt (n_rows values in tape row order, host or device, may be NULL) receives the new traveltimes.  Afterwards the tape is,
 *   bit for bit and in every result of every entry, the tape that ttcr_fsm_raytrace_multi_adjoint builds with the same grid, slowness and
 *   sources and with the moved receivers, followed by the same ttcr_fsm_rcv_points and ttcr_fsm_dd_pairs.  No field, coupling term,
 *   mask or frozen list changes.  A held cotangent is released as by ttcr_fsm_adjoint_release (its adjoint belonged to the old
 *   stencils); the point map, the pairs and every work array stay.  Every point has to be finite and has to pass the bounds check the
 *   raytrace entries apply to a receiver ("Receiver outside grid"), else TTCR_ERR_VALUE before any device write and the tape is unchanged.
 *   The first move gives both lists room for 8 entries per row and allocates three index arrays of that length and the sort's workspace;
 *   ttcr_fsm_adjoint_bytes reports them, TTCR_ERR_DEVICE with the byte count if that fails, ttcr_fsm_adjoint_free returns them.  Later
 *   moves allocate nothing.
 * ttcr_fsm_reloc_get_points: pts (3 n_rcv_points doubles) receives the current user coordinates of the receiver points: the values of the
 *   last move, or, before any move (and after ttcr_fsm_rcv_points replaced the map), the receiver of the point's first row with the
 *   origin of a translated grid added again in the grid dtype; NaN for a point without rows that no move has placed.
 * ttcr_fsm_reloc_gn: out_rcv = C G^T B (G C v_rcv), 4 n_rcv_points values: G is ttcr_fsm_rcv_jvp's operator, C = diag(rcv_scale) (NULL:
 *   none), B the row operator of ttcr_fsm_dd_apply's mode 2 (pair_weight NULL: diag(row_weight), NULL: the identity).  The kernels of
 *   ttcr_fsm_rjoint_gn without its two relaxations; its bits are those of ttcr_fsm_rjoint_gn's out_rcv for v = 0 (the sign of a zero
 *   may differ).
 * ttcr_fsm_reloc_solve: (C G^T B G C + diag(rcv_damp)) z = C rhs_rcv by the conjugate gradients of ttcr_fsm_rjoint_solve on a vector
 *   that is the receiver block alone (n_joint = 4 n_rcv_points): the same scaling, damping of the scaled unknown, inner products,
 *   recurrence, statuses and outputs; x_rcv = C z.  No relaxation in any iteration.  With pure double-difference data (row_weight all
 *   zero) and no damping of t0 the system is singular: the common origin-time shift is in the null space of Q.  The first call allocates
 *   five vectors of n_joint values and three of the block; ttcr_fsm_rcv_release returns them.
 * Pairs go straight into these two entries (pair_weight); the `system` argument of ttcr_fsm_dd_gn / ttcr_fsm_dd_solve stays 0 .. 2.
 * Argument errors return TTCR_ERR_VALUE naming the argument before any device call.  Two new kernels (a thread per row; a thread per
 * seed entry) and the device radix sort; everything else is the existing kernels.  No floating-point atomics.  Not covered: a direct
 * 4 x 4 solve per point, moving source points, S-P rows, 2-D, WENO, tt_from_rp = 1. */
int ttcr_fsm_reloc_move(ttcr_fsm_adjoint* t, const void* pts, int pts_on_device, void* tt, int tt_on_device);
int ttcr_fsm_reloc_get_points(const ttcr_fsm_adjoint* t, double* pts);
int ttcr_fsm_reloc_gn(const ttcr_fsm_adjoint* t, const void* v_rcv, int vr_on_device, const void* row_weight, int rw_on_device,
                      const void* pair_weight, int pw_on_device, const double* rcv_scale, void* out_rcv, int or_on_device);
int ttcr_fsm_reloc_solve(ttcr_fsm_adjoint* t, const void* rhs_rcv, int rr_on_device, const void* row_weight, int rw_on_device,
                         const void* pair_weight, int pw_on_device, const double* rcv_damp, const double* rcv_scale, int maxiter,
                         double rtol, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq);

/* Replaces: Grid2D::raytrace(Tx, t0, Rx, traveltimes, l_data, threadNo) (ttcr/Grid2D.h:616-640) and the overload with r_data
 * AND l_data (:583-614) -> Grid2Drn::getRaypath(Tx, t0, Rx, [r_data,] l_data, tt, threadNo) (ttcr/Grid2Drn.h:1852-2190): what
 * `compute_L=True` of the Python layer reaches for 2-D grids with cell slowness (src/ttcrpy/rgrid.pyx:3889-3893, :4060-4143).
 * One call solves the source in `slot`, walks every receiver's ray on the device and keeps, per receiver, the (cell index,
 * segment length) entries of the ray-projection matrix L, sorted by cell with the reference's comparator (CompareSiv_i,
 * ttcr/ttcr_t.h:417-422).  Restated AS IT STANDS: this walk gives up where the plain raypath walk retries along a face
 * ("going outside grid"); when the last two segments of a ray lie in one cell the reference pushes the entry of the first
 * AND an entry holding the sum, and the overload without r_data prices the last hop with that sum.  Traveltimes are those
 * of the overload (with_rays selects which).  Bit-identical to the compiled reference (tests/golden/l_golden.npz,
 * tests/test_l_matrix.py).  2-D grids with cell slowness only (TTCR_ERR_UNSUPPORTED otherwise: in 3-D ttcrpy itself raises
 * "compute_L defined for the FSM", rgrid.pyx:916-917; node grids: rgrid.pyx:3889-3890).
 * ttcr_fsm_slot_l_size: rows (= receivers) and entries of the last call on `slot`; ttcr_fsm_get_slot_l: row_off[n_rows+1],
 * cell[nnz] cell indices (x-major, z fastest, like Grid2Drn::getCellNo), v[nnz] lengths of the grid dtype.  With with_rays != 0
 * the rays of the call are available through ttcr_fsm_slot_rays_size / ttcr_fsm_get_slot_rays (two coordinates per point). */
int ttcr_fsm_raytrace_l(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx,
                        const void* rx, void* tt_out, int with_rays);
int ttcr_fsm_slot_l_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz);
int ttcr_fsm_get_slot_l(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* cell, void* v);
/* The same for every source of a call -- Grid2D's multi-source overloads with l_data (they run the single-source overload per source
 * on host threads), what ttcrpy reaches with compute_L and several events.  Sources and receivers laid out like
 * ttcr_fsm_raytrace_multi; batched solves, the walks follow each batch; results identical to n_src calls of ttcr_fsm_raytrace_l.
 * ONE CSR over all receiver rows of the call (ttcr_fsm_multi_l_size / ttcr_fsm_get_multi_l); with_rays != 0: the rays of the call
 * through ttcr_fsm_rays_size / ttcr_fsm_get_rays. */
int ttcr_fsm_raytrace_multi_l(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                              const void* rx, void* tt_out, int with_rays);
int ttcr_fsm_multi_l_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz);
int ttcr_fsm_get_multi_l(const ttcr_fsm_grid* g, long long* row_off, long long* cell, void* v);

typedef struct {
    double sweep_ms;        /* HIP-event time of all sweep launches of the last raytrace call   */
    double total_ms;        /* wall time of the last raytrace call (host clock, incl. copies)  */
    long long kernel_launches; /* sweep-tile kernel launches in the last call                  */
    long long node_updates;    /* nodes * 8 (or 4) * iterations, summed over sources           */
    long long evaluated_updates; /* node updates actually evaluated (chunks whose inputs did not
                                    change since their last evaluation are skipped, exactly)   */
    int iterations;         /* max sweep-iterations over the sources of the last call          */
    int n_sources;
} ttcr_fsm_timing;
int ttcr_fsm_last_timing(const ttcr_fsm_grid* g, ttcr_fsm_timing* out);
/* Decisions of the stopping rule since the grid was created: iterations decided by the reference's sequential sum, iterations
 * that landed in the window without a snapshot (decided by the fp64 sum), rounds of the parallel sum.  Any pointer may be NULL. */
int ttcr_fsm_stopping_stats(const ttcr_fsm_grid* g, long long* reference_sums, long long* reference_sums_missed, long long* rounds);
/* Calls (solve batches) that found their traveltime fields initialised by the side stream instead of filling them (option "prefill";
 * the fill it replaces: `reinit` of every node, ttcr/Grid3Drnfs.h:92-94).  No reference equivalent: tests and bench.py read it. */
int ttcr_fsm_prefill_swaps(const ttcr_fsm_grid* g, long long* swaps);
/* Calls whose first sweep launch re-initialised the other set of fields itself (option "prefill_inline") instead of leaving it to the side
 * stream.  No reference equivalent: tests read it. */
int ttcr_fsm_prefill_inline_fills(const ttcr_fsm_grid* g, long long* fills);
/* The reference's `change` (ttcr/Grid3Drnfs.h:141-152) of two fields given on the host, n_nodes values of the grid's type each, node
 * order: the sum, in node order, in T1, of abs(times[n] - field[n]), into *out (a T1).  parallel != 0: the parallel form the solver
 * uses; 0: one chain of additions.  Both exact; tests compare them. */
int ttcr_fsm_reference_change(ttcr_fsm_grid* g, const void* times, const void* field, int parallel, void* out);
/* Name of the sweep-kernel instantiation the last solve launched (first-order stage of the last batch; no reference
 * equivalent: bench.py reports it beside the roofline figures).  Written into buf (n bytes, NUL terminated). */
int ttcr_fsm_last_kernel(const ttcr_fsm_grid* g, char* buf, size_t n);
/* Test infrastructure, device free: the ticket order of the whole-iteration sweep launch of a grid with nnx x nny x nnz NODES (dim = 2:
 * nny is ignored), exactly the words the kernel reads -- one per work unit (sweep direction d, patch), TJ | TK << 14 | d << 28, with the
 * patch and chunk sizes the library uses for that dimension and dtype.  stage 0: first-order sweeps, 1: WENO sweeps (wider halo);
 * by_time 0: sweep by sweep, 1: by expected start time (the default of every launch).  The kernels are deadlock free with any number of
 * resident workgroups only if every unit comes after the units it waits for: tests/test_unit_order.py checks that.  *n_units: words
 * of the list; out may be NULL (size query), else capacity (in words) must be >= *n_units.  No reference equivalent. */
int ttcr_fsm_unit_order(int dim, int dtype, int stage, int by_time, uint32_t nnx, uint32_t nny, uint32_t nnz, uint32_t* out,
                        size_t capacity, size_t* n_units);
/* Test infrastructure, device free: the sweep kernel a grid of nnx x nny x nnz NODES (dim = 2: nny is ignored) with n_slots slots would launch
 * for `batch` batch entries (slot groups; slots with option mode = 0) in stage 0 (first-order sweeps) or 1 (WENO sweeps), exactly the
 * arithmetic of the solver (ttcr_amd/csrc/fsm_sweep_plan.h) under the TTCR_FSM_* variables of the environment.  keys / values: n_options
 * pairs as for ttcr_fsm_set_option -- "mode", "skip", "lone_chunk", "arith" -- and two that stand for what else a grid knows: "rotated"
 * (2-D rotated template with dx == dz) and "probe_skip" (0: the grid's last skipping solve evaluated too much, see SweepTuning).  wg_cap:
 * the workgroups a launch is capped at (a grid: 8 per compute unit of its device).  layout: -1, or 0 / 1 for a grid inside the window where
 * the layout follows the model (option "pair_layout").  name: what ttcr_fsm_last_kernel reports after such a launch.  out[12]:
 * [0] 0 the library holds that instantiation, 1 the launch is refused (option 'arith' without whole-iteration launches), 2 no such
 * instantiation; [1] workgroups, [2] threads per workgroup, [3] bytes of dynamic LDS, [4] ticket list (0 per sweep, 1 whole iteration
 * sweep by sweep, 2 by start time), [5] launches per sweep-iteration, [6] levels per chunk, [7] SKIP (2: every chunk taken for dirty),
 * [8] XS, [9] PRE, [10] fields per workgroup, [11] AR.  tests/test_sweep_plan.py.  No reference equivalent. */
int ttcr_fsm_sweep_plan(int dim, int dtype, int weno, uint32_t nnx, uint32_t nny, uint32_t nnz, int n_slots, const char* const* keys,
                        const double* values, int n_options, int wg_cap, int stage, int batch, int layout, char* name, size_t name_len,
                        long long* out);
/* Test infrastructure, device free: the dirty bits a changed node sets for the next sweep (ttcr_amd/csrc/fsm_chunk_dirty.h), exactly the
 * arithmetic of the first-order 3-D sweep kernels with exact skipping.  For every node (i, j, k) of a grid of nnx x nny x nnz NODES, as
 * if it had changed in the sweep of direction dir (0 .. 7), the units of the sweep after it -- direction (dir + 1) % 8, patches of THAT
 * direction's oriented partition, with the patch size the library uses for dtype and chunks of `chunk` (8 or 16) levels -- whose chunks
 * it marks: out[12 n .. 12 n + 11] for node n = (k nny + j) nnx + i holds up to three entries (TJ, TK, first chunk, last chunk), unused
 * entries -1.  edge_rule 0 leaves out the patches beyond a patch edge (a negative control for tests).  capacity: words of out, at least
 * 12 per node.  tests/test_chunk_dirty_marks.py.  No reference equivalent. */
int ttcr_fsm_chunk_dirty_marks(int dtype, int chunk, int dir, int edge_rule, uint32_t nnx, uint32_t nny, uint32_t nnz, int32_t* out, size_t capacity);
/* Test infrastructure, device free: the slice of the spare traveltime fields that the unit with ticket `ticket` of a launch of n_tickets
 * units sets to max() (option "prefill_inline"), exactly the arithmetic the kernel does (ttcr_amd/csrc/fsm_prefill_slices.h).  n_el:
 * elements of the spare set.  *slice_len: elements per ticket, a multiple of the 16-byte vector (4 fp32, 2 fp64 elements); [*begin, *end):
 * the ticket's elements -- tickets 0 .. n_tickets - 1 tile [0, n_el) in order without gap or overlap, tickets from n_tickets on are
 * empty.  Any pointer may be NULL.  tests/test_prefill_slices.py.  No reference equivalent. */
int ttcr_fsm_prefill_slice(int dtype, uint64_t n_el, uint32_t n_tickets, uint32_t ticket, uint64_t* slice_len, uint64_t* begin, uint64_t* end);
/* Build provenance: the 16-hex-digit hash of the kernel sources and compiler flags this library was compiled from (ttcr_amd/build.py,
 * source_hash(), baked in at compile time).  The Python layer refuses a library whose id is not the hash of the sources beside it, and
 * bench.py / the tests print it: a measured binary is provably the committed code.  "unknown" for a build that did not pass the id. */
const char* ttcr_fsm_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* TTCR_AMD_H */
