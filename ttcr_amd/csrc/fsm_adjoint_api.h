// ttcr_amd/csrc/fsm_adjoint_api.h -- the field tape (ttcr_fsm_raytrace_multi_adjoint, include/ttcr_amd.h): what the host side (fsm_capi.hip)
// sees of the kernels that back-propagate a cotangent through the first-order Godunov update of the 3-D node solver.  The kernels live in a
// translation unit of their own (fsm_adjoint.hip).  Definition: DESIGN.md 6b; tests/adjoint_reference.py restates it in numpy.
//
// Per tape, once:   frozen marks -> coupling pass (per node and event: D, the sum of the active upwind differences, and the 6-bit mask of the
//                   neighbours that have this node as an active upwind neighbour).
// Per JVP:          relaxation of mu = own term + gather(mu) over the at most three upwind neighbours (the same two schedules; the upwind
//                   choice is recomputed from the field) -> receiver rows through the stencil, one thread per row.
// Per HVP / Newton product: JVP relaxation -> dD (per node) -> q (gather through the in-mask, lam of the held cotangent)
//                   -> VJP relaxation seeded with q (and the weighted rows of J v) -> gradient with the direct term added.
// Per VJP:          seed (g = field cotangent + receiver rows through the interpolation stencil, one serial chain per node in row order)
//                   -> relaxation of lam = g + gather(lam) to its fixed point (tiled in LDS, or the global Jacobi baseline)
//                   -> gradient (events summed in ascending order from +0 inside the thread).
// Per block product: the same steps for groups of four model vectors, the four values of a node adjacent: K-column seeds,
//                   K-column relaxations (tiled; what a step needs of the field is read and formed once per node), K-column gradient.
// Normal equations (fsm_normal.hip): the smoothing operator on the model vector (a tile with a two-node halo in LDS), inner
//                   products summed in a fixed order (chunks of 1024, one finishing workgroup), and conjugate gradients around the
//                   Gauss-Newton / Newton product with the scalars of the recurrence formed on the device.  One solver (adj_solve) over
//                   four systems (CgSystem): the model vector alone, or with the source block (6j) or the receiver block (6k) behind it,
//                   or the receiver block alone (6o).
// Moving receivers: the rows' points, traveltimes, gradients and stencils from one kernel (a thread per row), the seed list
//                   of the adjoint from a stable device radix sort of the stencil entries and a gather -- no solve, no relaxation.
// Grid search (fsm_locate.hip): per hypocentre the node of the tape's fields with the smallest weighted, origin-time-corrected
//                   misfit of its picks -- one search kernel (partial minima per workgroup), one finishing kernel; no solve, no relaxation.
// No floating-point atomics anywhere: every value is one fixed expression of final values, so the bits do not depend on the schedule.
// Cell tapes (ttcr_fsm_raytrace_multi_adjoint_cells): the model vector holds one slowness per cell and the node slowness is
// A times it (fsm_cells_to_nodes3d); a jvp first applies A to ds, a vjp ends with A^T on the node gradient (one thread per cell).
// Model tapes (ttcr_fsm_model_raytrace_multi_adjoint; kernels in fsm_model.hip): the model vector holds the slowness at the
// nodes of a coarse grid and the node perturbation is P times it, P the trilinear prolongation; a jvp first applies P, a vjp ends with P^T.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <stdexcept>
#include <vector>

namespace ttcr_amd {

// an allocation or a copy of the tape failed on the device (the C ABI turns it into TTCR_ERR_DEVICE)
struct AdjDeviceError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// What the solves of a call leave for the tape.  The fields and the slowness go straight to device memory of `device` (allocated by the
// caller before the solves); the small lists are collected on the host.  Replicas of a multi-device grid fill disjoint events and rows.
struct AdjSink {
    int device = 0;
    size_t elem = 4, nn = 0;
    void* fields = nullptr;     // n_events * nn values: event e at fields + e * nn * elem
    void* slowness = nullptr;   // nn values (written with event 0)
    // frozen nodes of every event (fsm_init_source): node and distance d of the point that wrote it last (a T value, held exactly)
    std::vector<std::vector<int>> fr_node;
    std::vector<std::vector<double>> fr_d;
    // ... and, for the source derivative: the point that wrote the node last (index within the event, tx order) and
    // c[a] = fl(fl(p_a - x_a) / d) for a = x, y, z (+0 where d = 0), computed in T and held exactly; 3 values per node
    std::vector<std::vector<int>> fr_pt;
    std::vector<std::vector<double>> fr_c;
    std::vector<int> pt_off;    // n_events + 1: first point of every event among the points of the call
    bool cells = false;         // the call came through the cell entry: the grid has to be a cell grid (a node grid otherwise)
    // interpolation stencil of every receiver row (interp3d_stencil): 8 slots per row, st_cnt[row] of them used
    std::vector<int> st_cnt, st_event;
    std::vector<long long> st_node;
    std::vector<double> st_w;
    // ... and, for the receiver derivative: the receiver of every row as the solver sees it (after the origin shift of a
    // translated grid; T values held exactly, 3 per row), the origin the solver interpolates with and the shift of a translated grid
    std::vector<double> st_p;
    double rcv_min[3] = {0, 0, 0}, rcv_shift[3] = {0, 0, 0};
    // ... and the upper corner the solver checks a point against (after the shift), for a tape that moves its receivers
    double rcv_max[3] = {0, 0, 0};
};

// ---- the coarse model grid (tests/model_reference.py restates it; fsm_model.hip).  The per-axis tables of the trilinear
// prolongation P from m[0] x m[1] x m[2] model nodes onto n[0] x n[1] x n[2] fine nodes (both x fastest, 1 <= m[d] <= n[d]), on the
// current device: for every fine index of every axis the lower model index and the weights wl, wh in the grid dtype.
struct ModelMap {
    int n[3] = {0, 0, 0}, m[3] = {0, 0, 0};
    int* idx = nullptr;   // n[0] + n[1] + n[2]: x, then y, then z
    void* w = nullptr;    // twice as many values: wl of the three axes, then wh
    size_t bytes = 0;     // what the two arrays hold
    size_t n_fine() const { return (size_t)n[0] * n[1] * n[2]; }
    size_t n_model() const { return (size_t)m[0] * m[1] * m[2]; }
    // elements of the intermediates of P^T: after stage z and after stage y
    size_t n_stage_z() const { return (size_t)n[0] * n[1] * m[2]; }
    size_t n_stage_y() const { return (size_t)n[0] * m[1] * m[2]; }
};
size_t model_map_bytes(const int n[3], size_t elem);
// the stencil of fine index i on an axis of n fine and m model nodes: lower model index and the two quotients in double
void model_axis_stencil(int i, int n, int m, int* I, double* wl, double* wh);
// forms the tables on the host and uploads them (blocking copies); AdjDeviceError naming the byte count if an allocation fails
template <typename T>
void model_map_create(ModelMap& map, const int n[3], const int m[3]);
void model_map_free(ModelMap& map);
// d_s (n_fine()) = P d_v (n_model()): one kernel, one thread per fine node
template <typename T>
void model_prolong(const ModelMap& map, const T* d_v, T* d_s, hipStream_t stream);
// d_gm (n_model()) = P^T d_g (n_fine()) in three stages, z first, through d_a (n_stage_z()) and d_b (n_stage_y()): serial sums in
// ascending order, one thread per output element, no atomics
template <typename T>
void model_restrict(const ModelMap& map, const T* d_g, T* d_a, T* d_b, T* d_gm, hipStream_t stream);

// The systems the conjugate-gradient solver of fsm_normal.hip runs on: the model vector alone, the model vector followed by
// the source block (the joint hypocentre-velocity system, 6j), or followed by the receiver block (the receiver joint system, 6k) -- or the
// receiver block alone, its model block empty (the relocation-only system, 6o).
enum CgSystem { CG_MODEL = 0, CG_SOURCE = 1, CG_RECEIVER = 2, CG_RELOC = 3 };
constexpr int CG_SYSTEMS = 4;
// the work arrays of the solver for one system, all on the tape's device; n = cg_len(system), b = cg_block(system)
struct CgWork {
    void* x = nullptr;        // n each: the iterate (a host x0 and the host result are staged here; its block in the scaled unknown z_e), ...
    void* r = nullptr;        // ... the residual (the rhs goes here; model system: a host operand of dot, a host v of smooth), ...
    void* p = nullptr;        // ... the search direction (model system: the second host operand of dot), ...
    void* q = nullptr;        // ... A p (model system: a host result of smooth is staged here) ...
    void* hp = nullptr;       // ... and the output of the tape's product
    void* scale = nullptr;    // b each, only for a system with a block: the column scaling c, the damping delta of the block, ...
    void* damp = nullptr;
    void* ve = nullptr;       // ... and fl(c * p_e) of the running product
    void* partial = nullptr;  // one double per chunk of 1024 elements
    void* ctl = nullptr;      // the scalars of the recurrence
    size_t bytes = 0;         // what these arrays added to total_bytes
};

struct AdjTapeDev {
    int device = 0;
    size_t elem = 0, n_events = 0, n_rows = 0, nn = 0;
    int nnx = 0, nny = 0, nnz = 0;
    double dx = 0;
    // cell tape: the model vector of vjp / jvp / gn holds nc = (nnx - 1) (nny - 1) (nnz - 1) cell values (x fastest) instead of nn node values
    bool cells = false;
    size_t nc = 0;
    void* cell_tmp = nullptr;         // n_model() (cell and model tapes only: a host grad / ds / v / out is staged here; grad_tmp holds the node vector)
    // model tape: the model vector holds the map.n_model() values of a coarse node grid, the node vector is P times it
    bool model = false;
    ModelMap map;                     // the axis tables of P (counted in total_bytes)
    void* map_a = nullptr;            // the intermediates of P^T: map.n_stage_z() values ...
    void* map_b = nullptr;            // ... and map.n_stage_y()
    bool mapped() const { return cells || model; }   // the model vector is not the node vector: a linear map stands between them
    size_t n_model() const { return cells ? nc : (model ? map.n_model() : nn); }
    void* model_tmp() const { return mapped() ? cell_tmp : grad_tmp; }
    void* fields = nullptr;           // n_events * nn
    void* slowness = nullptr;         // nn
    void* D = nullptr;                // n_events * nn: D of a non-frozen node, d of a frozen one
    unsigned char* inmask = nullptr;  // n_events * nn: bit 2 * axis + side (x-, x+, y-, y+, z-, z+): that neighbour feeds this node
    unsigned char* frozen = nullptr;  // n_events * nn: 1 = frozen
    void* g = nullptr;                // n_events * nn: the seeds of the running VJP
    void* lam = nullptr;              // n_events * nn
    void* lam2 = nullptr;             // n_events * nn: second buffer of the Jacobi baseline; a host field cotangent is staged here
    size_t n_seed = 0;                // stencil entries, sorted by (event, node), rows ascending within a node
    long long* sd_key = nullptr;      // event * nn + node
    int* sd_row = nullptr;
    void* sd_w = nullptr;
    int* flags = nullptr;             // ring of per-event "a value changed in pass p" flags
    int* stamps = nullptr;            // per event and tile: the last pass that changed the tile
    int* err = nullptr;               // internal error flag of the coupling pass
    void* w_tmp = nullptr;            // n_rows (host w staged here)
    void* grad_tmp = nullptr;         // nn (host grad staged here; a host ds of the forward mode too)
    // forward mode (allocated and uploaded by the first jvp): the stencil entries in row order, and a staging row for a host row_weight
    int* rw_off = nullptr;            // n_rows + 1: entries of row r at rw_off[r] .. rw_off[r + 1]
    long long* rw_key = nullptr;      // event * nn + node
    void* rw_w = nullptr;
    void* rw_tmp = nullptr;           // n_rows
    int* tan_stamps = nullptr;        // per event and tangent tile: the last pass that changed the tile
    size_t n_tan_tiles = 0;
    std::vector<int> h_rw_off;        // host copies, kept from adj_finish on
    std::vector<long long> h_rw_key;
    std::vector<double> h_rw_w;
    // source derivative.  Host lists, kept from adj_finish on: the frozen entries sorted by (point, node) -- a node belongs
    // to the point that wrote it last --, uploaded by the first jvp_source / vjp_source
    size_t n_points = 0;
    std::vector<int> h_pt_event;      // n_points: event of every point
    std::vector<int> h_src_off;       // n_points + 1: entries of point q at h_src_off[q] .. h_src_off[q + 1]
    std::vector<long long> h_src_key; // event * nn + node
    std::vector<double> h_src_c;      // 3 per entry
    int* src_off = nullptr;
    int* src_pt = nullptr;            // point of every entry
    long long* src_key = nullptr;
    int* src_node = nullptr;
    void* src_c = nullptr;
    void* src_io = nullptr;           // 16 n_points values: a host dsrc / gsrc is staged here
    void* src_rows = nullptr;         // 4 n_rows values: the dtt of a K-column call before it goes to the host
    void* mu4 = nullptr;              // 4 n_events * nn: the four columns of a node adjacent (allocated by the first call with n_cols > 1)
    void* mu4b = nullptr;             // second buffer of the Jacobi baseline (allocated by the first such call with that schedule)
    // second-order products: allocated by hold, returned by release_hold
    void* hold_lam = nullptr;         // n_events * nn: lam of the held cotangent
    void* hess_dd = nullptr;          // n_events * nn: dD of the running product
    bool held = false;                // hold_lam holds a solved lam
    // block products: allocated by the first block call, returned by adj_block_release.  lam of K columns lives in mu4.
    void* g4 = nullptr;               // 4 n_events * nn: the seeds of the running K-column vjp (a host dfields of jvp_block is staged here)
    void* blk_model = nullptr;        // 4 n_model(): a group of host ds / v / grad / out columns
    void* blk_nodes = nullptr;        // 4 nn (cell and model tapes only): the node vectors of a group
    void* blk_rows = nullptr;         // 4 n_rows: a group of host w / dtt columns; J v of a Gauss-Newton group
    void* blk_rw = nullptr;           // 4 n_rows: a group of host row_weight columns
    bool blk_owns_mu4 = false;        // mu4 came with the block arrays (no jvp_source had allocated it) and leaves with them
    size_t blk_bytes = 0;             // what the block arrays added to total_bytes
    // the conjugate-gradient solver: one set of work arrays per system, allocated by the first call that needs it
    // (smooth, dot or solve for the model system; the first solve for the other two) and returned by adj_cg_release
    CgWork cg[CG_SYSTEMS];            // by CgSystem
    // elements of a system's extra block, (t0, x, y, z) of every source point in call order or of every receiver point, of its model
    // block (empty for the relocation-only system) and of its vector: the model block, then the extra block
    size_t cg_block(CgSystem s) const { return s == CG_MODEL ? 0 : 4 * (s == CG_SOURCE ? n_points : n_rcv_points); }
    size_t cg_model(CgSystem s) const { return s == CG_RELOC ? 0 : n_model(); }
    size_t cg_len(CgSystem s) const { return cg_model(s) + cg_block(s); }
    // receiver points.  Host lists, kept from adj_finish on: the receiver of every row as the solver sees it, the point of
    // every row (default: one point per row) and the rows of every point (CSR, rows ascending within a point).  The first receiver call
    // uploads them, evaluates G of the tape's rows and allocates the staging arrays; adj_rcv_release returns all of it
    std::vector<double> h_rcv_p;      // 3 n_rows
    std::vector<int> h_rcv_event;     // n_rows
    std::vector<int> h_rcv_pt;        // n_rows: receiver point of every row
    std::vector<int> h_rcv_off;       // n_rcv_points + 1: rows of point q at h_rcv_rows[h_rcv_off[q] .. h_rcv_off[q + 1])
    std::vector<int> h_rcv_rows;      // n_rows
    size_t n_rcv_points = 0;
    double rcv_min[3] = {0, 0, 0};    // the origin the solver interpolates with
    double rcv_shift[3] = {0, 0, 0};  // what a translated grid subtracts from a point first (zeros otherwise)
    double rcv_max[3] = {0, 0, 0};    // the upper corner the solver checks a shifted point against
    void* rcv_p = nullptr;            // 3 n_rows
    int* rcv_event = nullptr;         // n_rows
    int* rcv_pt = nullptr;            // n_rows
    int* rcv_off = nullptr;           // n_rcv_points + 1
    int* rcv_rows = nullptr;          // n_rows
    void* rcv_G = nullptr;            // 3 n_rows: d tt[row] / d (x, y, z) of its receiver
    void* rcv_tt = nullptr;           // n_rows: interp3d_pt of the tape's rows (a host dtt of jvp_rcv is staged here too)
    void* rcv_io = nullptr;           // 16 n_rcv_points values: a host drcv / grcv is staged here (four blocks, as src_io)
    size_t rcv_bytes = 0;             // what these arrays added to total_bytes
    void* rcv_stage = nullptr;        // staging of rcv_eval at arbitrary points: grow-only, returned by adj_rcv_release
    size_t rcv_stage_bytes = 0;
    // moving the receiver points.  The first move gives the seed list (sd_*) and the row-order list (rw_key, rw_w) room
    // for mv_cap = 8 n_rows entries -- a row has 1, 2, 4 or 8 -- and allocates what the rebuild on the device works in; all of it stays
    // until the tape is freed.  h_mv_pts: the points of the last move as the caller gave them (T values held exactly, 3 per receiver
    // point; empty before the first move and after adj_rcv_set_points)
    size_t mv_cap = 0;
    int* mv_row = nullptr;            // mv_cap: the row of every entry of the row-order list
    int* mv_idx = nullptr;            // mv_cap: 0, 1, 2, ... (the values the sort carries)
    int* mv_perm = nullptr;           // mv_cap: the entry of the row-order list that stands at each place of the seed list
    void* mv_sort = nullptr;          // the radix sort's workspace
    size_t mv_sort_bytes = 0;
    std::vector<double> h_mv_pts;
    // grid search: the uploaded picks, the partial minima and the results of a call, and the misfit volume of a call that
    // wants it on the host; both grow to the largest call and are returned by adj_loc_release
    void* loc_work = nullptr;
    size_t loc_work_bytes = 0;
    void* loc_vol = nullptr;
    size_t loc_vol_bytes = 0;
    // double-difference rows.  Host lists, kept from adj_dd_set_pairs on: the two tape rows of every pair in the caller's order
    // and the pairs of every row (CSR, ascending pair index within a row, one int per entry: 2 p + sign, sign 1 for the row that is
    // subtracted).  The first call that uses pairs uploads them and allocates the three work arrays; adj_dd_release returns all of it
    bool dd_set = false;              // adj_dd_set_pairs has run (an empty list counts)
    size_t n_pairs = 0;
    std::vector<int> h_dd_a, h_dd_b;  // n_pairs each
    std::vector<int> h_dd_off;        // n_rows + 1
    std::vector<int> h_dd_ent;        // 2 n_pairs
    int* dd_a = nullptr;
    int* dd_b = nullptr;
    int* dd_off = nullptr;
    int* dd_ent = nullptr;
    void* dd_u = nullptr;             // n_pairs: d or u of the running product (a host result of Q x is staged here)
    void* dd_pw = nullptr;            // n_pairs: a host pair_weight (or the host y of Q^T y) is staged here
    void* dd_rows = nullptr;          // n_rows: B w of the running product (a host result of Q^T y / B x is staged here)
    size_t dd_bytes = 0;              // what these arrays added to total_bytes
    size_t n_tiles = 0;
    size_t total_bytes = 0;
    hipStream_t stream = nullptr;
    size_t bytes() const { return total_bytes; }
    void release();
};

// edge of a relaxation tile (interior nodes) for an element size
int adj_tile_edge(size_t elem);
int adj_tan_tile_edge(size_t elem);   // the forward mode's
// allocates fields and slowness (what the solves write into); throws AdjDeviceError naming the byte count
void adj_alloc_fields(AdjTapeDev& t);
// strided field (element n at src[n * ts]) -> contiguous dst, both on the current device
template <typename T>
void adj_copy_field(const T* src, int ts, T* dst, size_t n, hipStream_t stream);
// uploads the lists of the sink, allocates the work arrays, marks the frozen nodes and runs the coupling pass
template <typename T>
void adj_finish(AdjTapeDev& t, const AdjSink& sink);
// d_w (n_rows, may be null), d_fc (n_events * nn, may be null), d_grad (n_model()): all on the tape's device; returns the passes launched.
// On a cell tape the node gradient is formed in grad_tmp and d_grad = A^T grad_tmp; on a model tape d_grad = P^T grad_tmp.
template <typename T>
int adj_vjp(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule);
// forward mode (tests/tangent_reference.py restates it): d_ds (n_model(); a cell tape relaxes with grad_tmp = A d_ds, a model tape with P d_ds), d_dtt
// (n_rows, may be null), d_dfields (n_events * nn, may be null); relaxes mu = dT/ds . ds in lam / lam2 to its fixed point (the same two schedules), then one thread per receiver row; returns the
// passes launched.  The first call allocates adj_jvp_extra_bytes(t) more (AdjDeviceError naming the byte count if that fails).
size_t adj_jvp_extra_bytes(const AdjTapeDev& t);
template <typename T>
void adj_jvp_prepare(AdjTapeDev& t);   // that allocation and the upload of the row-order stencil; a no-op from the second call on
template <typename T>
int adj_jvp(AdjTapeDev& t, const T* d_ds, T* d_dtt, T* d_dfields, int schedule);

// ---- double-difference rows (tests/dd_reference.py restates them).  The data operator of a product is
// B = diag(rw) + Q^T diag(pw) Q, row p of Q holding +1 at tape row a_p and -1 at tape row b_p.
// replaces the pair list (rows already checked: a != b, both below n_rows, at most 2^30 - 1 pairs) and rebuilds the CSR by row; frees
// what the pair calls hold on the device (the next call uploads the new list).  Host only apart from that.
void adj_dd_set_pairs(AdjTapeDev& t, const int* row_a, const int* row_b, size_t n_pairs);
// what the first call that uses pairs adds to the tape; adj_dd_prepare is a no-op while it is there (AdjDeviceError naming the byte count
// if an allocation fails); adj_dd_release frees it and takes it off bytes().  The pairs stay as set.
size_t adj_dd_bytes(const AdjTapeDev& t);
void adj_dd_prepare(AdjTapeDev& t);
void adj_dd_release(AdjTapeDev& t);
// mode 0: d_out (n_pairs) = Q d_x, d[p] = fl(x[a_p] - x[b_p]).  mode 1: d_out (n_rows) = Q^T d_x, d_x holding n_pairs values: per row
// a chain from +0 over its entries in ascending p, acc = fl(acc +- y[p]).  mode 2: d_out (n_rows) = B d_x: u[p] = fl(pw[p] * d[p]) (d_pw
// null: d[p]) into dd_u, then per row the chain from fl(rw[r] * x[r]) (d_rw null: from x[r]) over u.  d_x and d_out are different arrays.
template <typename T>
void adj_dd_apply(AdjTapeDev& t, int mode, const T* d_x, const T* d_rw, const T* d_pw, T* d_out);
// The data weighting of a product: rw (n_rows, may be null) alone is today's diagonal; with pw (n_pairs) the operator B above.
template <typename T>
struct RowOp {
    const T* rw = nullptr;
    const T* pw = nullptr;
};
// applies op to the rows d_w (n_rows) and returns the array that holds the result: without pw, d_w itself, scaled in place by rw (or
// untouched); with pw, dd_rows.
template <typename T>
const T* adj_row_operator(AdjTapeDev& t, const RowOp<T>& op, T* d_w);

// Gauss-Newton product: jvp into w_tmp -> the row operator (RowOp: w_tmp *= rw, or B w_tmp into dd_rows) -> vjp into d_out (n_model()),
// all on the tape's stream
template <typename T>
void adj_gn(AdjTapeDev& t, const T* d_v, const RowOp<T>& op, T* d_out, int schedule, int* passes_jvp, int* passes_vjp);

// ---- second-order products (tests/hessian_reference.py restates them)
// hold: the vjp of (d_w, d_fc) -- d_grad (n_model(), may be null) with the bits of adj_vjp -- whose lam stays on the tape in hold_lam; the
// first hold allocates adj_hold_bytes(t) (hold_lam and the dD workspace; AdjDeviceError naming the byte count if that fails), a later one
// replaces the held lam.  adj_release_hold frees both and takes them off bytes().
size_t adj_hold_bytes(const AdjTapeDev& t);
template <typename T>
int adj_hold(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, int schedule);
void adj_release_hold(AdjTapeDev& t);
// d_out (n_model()) = the derivative in direction d_v (n_model()) of the held vjp with (w, field_cot) fixed; newton: plus J^T (d_rw * J v)
// (the row operator op, as in adj_gn) from the same adjoint relaxation.  d_v and d_out may be the same array.  Throws
// std::invalid_argument without a held cotangent.  Uses g, lam, lam2, w_tmp (and grad_tmp on a cell tape) as jvp and vjp do.
template <typename T>
void adj_hess(AdjTapeDev& t, const T* d_v, const RowOp<T>& op, bool newton, T* d_out, int schedule, int* passes_jvp, int* passes_vjp);

// ---- derivatives with respect to the source points (tests/source_reference.py restates them)
// what the first jvp_source / vjp_source adds to the tape (the lists above and the two staging arrays), and what the first call with
// n_cols > 1 adds per K-column buffer
size_t adj_src_extra_bytes(const AdjTapeDev& t);
size_t adj_src_column_bytes(const AdjTapeDev& t);
template <typename T>
void adj_src_prepare(AdjTapeDev& t);   // a no-op from the second call on
// d_dsrc (n_cols * n_points * 4), d_dtt (n_cols * n_rows, may be null), d_dfields (n_cols * n_events * nn, may be null): on the tape's
// device.  One relaxation of K = 1 (n_cols = 1) or K = 4 columns (the columns past n_cols are +0); returns the passes launched.
// *mu_out (may be null) receives the relaxed buffer: n_events * nn * K values, the K columns of a node adjacent; *k_out its K.
template <typename T>
int adj_jvp_source(AdjTapeDev& t, const T* d_dsrc, int n_cols, T* d_dtt, T* d_dfields, int schedule, const T** mu_out, int* k_out);
// the vjp (d_grad may be null here) and, from the same lam, d_gsrc (n_points * 4)
template <typename T>
int adj_vjp_source(AdjTapeDev& t, const T* d_w, const T* d_fc, T* d_grad, T* d_gsrc, int schedule);


// ---- block products: groups of up to 4 model vectors per relaxation.  Column k of every result has the bits of the
// one-column call (adj_jvp / adj_vjp / adj_gn) on column k.
// What the first block call adds to the tape: the K-column seeds g4 (4 n_events nn), the K-column lam / mu buffer mu4 (as much again, unless
// a jvp_source with n_cols > 1 allocated it before) and the staging arrays of a group (4 n_model(), 4 nn on a cell or model tape, 8 n_rows); the
// first jvp's arrays too if no jvp came before.  AdjDeviceError naming the byte count if an allocation fails.
size_t adj_block_bytes(const AdjTapeDev& t);
template <typename T>
void adj_block_prepare(AdjTapeDev& t);   // a no-op while the arrays are there
void adj_block_release(AdjTapeDev& t);   // frees them (mu4 only if it came with them) and takes them off bytes()
// one group, n_cols from 1 to 4, every array on the tape's device, column k at k * (length of one column): d_ds (n_cols x n_model()),
// d_dtt (n_cols x n_rows, may be null), d_dfields (n_cols x n_events * nn, may be null; may be g4); d_w (n_cols x n_rows), d_grad (n_cols x
// n_model()); d_rw: column k of the row weights at d_rw + k * rw_stride (null: none; rw_stride 0: one set shared by the columns).
// schedule 0 relaxes the group at once (K = 4, the columns past n_cols +0), schedule 1 runs the columns one by one through the Jacobi
// baseline.  Return the passes launched.
template <typename T>
int adj_jvp_block(AdjTapeDev& t, const T* d_ds, int n_cols, T* d_dtt, T* d_dfields, int schedule);
template <typename T>
int adj_vjp_block(AdjTapeDev& t, const T* d_w, int n_cols, T* d_grad, int schedule);
template <typename T>
void adj_gn_block(AdjTapeDev& t, const T* d_v, const T* d_rw, size_t rw_stride, int n_cols, T* d_out, int schedule, int* passes_jvp,
                  int* passes_vjp);

// ---- normal equations (tests/normal_reference.py restates them; kernels in fsm_normal.hip).  Model vectors are n_model()
// values on the tape's device, parameters x fastest: nnx x nny x nnz nodes, the (nnx - 1) x (nny - 1) x (nnz - 1) cells of a cell tape, or
// the model nodes of a model tape (spacing per axis dx (nn_d - 1) / (m_d - 1); an axis with fewer than 3 model nodes is left out of R and
// has to have weight 0).
// d_nodes (nn) = the map of the tape (A or P) applied to d_model (n_model()), and d_model = its transpose applied to d_nodes; on the
// tape's stream.  Node tapes have no map (std::logic_error).
template <typename T>
void adj_model_to_nodes(AdjTapeDev& t, const T* d_model, T* d_nodes);
template <typename T>
void adj_nodes_to_model(AdjTapeDev& t, const T* d_nodes, T* d_model);
// what is wrong with the smoothing weights on this tape (null: nothing): host only
const char* adj_smooth_error(const AdjTapeDev& t, const double* weights);
int adj_smooth_tile_edge(size_t elem);   // edge of a smoothing tile (interior parameters) for an element size
// the work arrays of the solver for one system (CgWork): five vectors of cg_len(sys) values, one double per chunk of 1024 elements and the
// scalars; for a system with a block three arrays of cg_block(sys) values more.  adj_cg_prepare is a no-op while they are there
// (AdjDeviceError naming the byte count if an allocation fails); adj_cg_release frees them and takes them off bytes().  adj_smooth's host
// staging and adj_dot use the model system's.
size_t adj_cg_bytes(const AdjTapeDev& t, CgSystem sys);
void adj_cg_prepare(AdjTapeDev& t, CgSystem sys);
void adj_cg_release(AdjTapeDev& t, CgSystem sys);
// d_out = R d_v = sum_d weights[d] K_d^T (K_d d_v), K_d the second differences of spacing dx along axis d with the centred stencil
// shifted inwards on the two end rows; d_out and d_v are different arrays.  std::invalid_argument with adj_smooth_error's words.
template <typename T>
void adj_smooth(AdjTapeDev& t, const T* d_v, const double* weights, T* d_out);
// <d_a, d_b> in fp64 with the fixed summation order of DESIGN.md 6i (chunks of 1024, one finishing workgroup); waits for the stream
template <typename T>
double adj_dot(AdjTapeDev& t, const T* d_a, const T* d_b);
// A = H + smooth R + damp I with H the Gauss-Newton product (newton: the Newton product of the held cotangent); a term whose factor is
// 0 is not evaluated
struct NormalOperator {
    double smooth = 0, damp = 0;
    double weights[3] = {1, 1, 1};
    bool newton = false;
};
struct NormalResult {
    int status = 1;                 // 0: the residual test was met; 1: maxiter iterations without meeting it; 2: <p, A p> not positive
    int iterations = 0;             // completed updates of x
    std::vector<double> rho;        // <rhs, rhs>, <r, r> of the starting residual, then <r, r> after every completed iteration
    std::vector<double> pq;         // <p, A p> of every iteration that evaluated it
    std::vector<int> passes;        // (jvp, vjp) passes of the product of every such iteration
    int passes0[2] = {0, 0};        // ... and of A x0
};
// Conjugate gradients on A x = rhs for one of the four systems, w = t.cg[sys]: on entry w.r holds rhs (its block unscaled) and, if
// with_x0, w.x holds x0; on return w.x holds the iterate.  rop: the row operator of the products, on the tape's device.  Vectors in T, scalars in
// fp64, inner products as adj_dot over the flat vector of the system; one host read of the scalars per iteration.  What differs between
// the systems: the product (adj_gn, or adj_hess if op.newton, for CG_MODEL; adj_gn_joint for CG_SOURCE; adj_gn_rjoint for CG_RECEIVER; adj_gn_reloc for CG_RELOC, whose model block is empty) and
// the block -- w.scale / w.damp hold c and delta if with_scale / with_damp, the block of rhs is scaled by c before the loop and the block
// of x after it (x_e = fl(c * z_e)), and the block of A p is fl(hp + fl(delta * p)).  x0 and op.newton are offered for CG_MODEL only
// (std::invalid_argument otherwise), a scale and a block damping only for the other two.
template <typename T>
void adj_solve(AdjTapeDev& t, CgSystem sys, const RowOp<T>& rop, const NormalOperator& op, bool with_x0, bool with_scale, bool with_damp,
               int maxiter, double rtol, int schedule, NormalResult& res);

// ---- joint hypocentre-velocity products (tests/joint_reference.py restates them and the solve).  Source blocks are 4 n_points
// values, (t0, x, y, z) of every point in call order, on the tape's device.
// the joint tangent of (d_ds, d_dsrc) from ONE relaxation: the frozen nodes are seeded with fl(fl(d ds) + sigma), every other node obeys
// the forward mode's system; outputs as adj_jvp.  *mu_out (may be null) receives the relaxed buffer.  Returns the passes launched.
template <typename T>
int adj_jvp_joint(AdjTapeDev& t, const T* d_ds, const T* d_dsrc, T* d_dtt, T* d_dfields, int schedule, const T** mu_out);
// (d_gs, d_ge) = [J_s J_e C]^T (op [J_s J_e C] (d_vs, d_ve)), op the row operator as in adj_gn, C = diag(d_scale) (null: no scaling, no multiplication); d_ve_scaled (4
// n_points, unused without a scale) receives fl(c * d_ve).  d_gs has the bits of adj_vjp_source's gradient, d_ge = fl(c * its gsrc).
template <typename T>
void adj_gn_joint(AdjTapeDev& t, const T* d_vs, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_gs, T* d_ge,
                  int schedule, int* passes_jvp, int* passes_vjp);

// ---- derivatives with respect to the receiver points (tests/receiver_reference.py restates them).  Receiver blocks are 4
// n_rcv_points values, (t0, x, y, z) of every receiver point, on the tape's device.
// replaces the map row -> receiver point (tape row order; n_points >= every value + 1) and rebuilds the CSR by point; frees what the
// receiver calls hold on the device (the next call uploads the new map).  Host only apart from that.
void adj_rcv_set_points(AdjTapeDev& t, const int* point_of_row, size_t n_points);
// what the first receiver call adds to the tape; adj_rcv_prepare is a no-op while it is there (AdjDeviceError naming the byte count if
// an allocation fails); adj_rcv_release frees it and the solver's arrays of the receiver system and takes them off bytes()
size_t adj_rcv_extra_bytes(const AdjTapeDev& t);
template <typename T>
void adj_rcv_prepare(AdjTapeDev& t);
void adj_rcv_release(AdjTapeDev& t);
// the staging buffer of rcv_eval at arbitrary points, at least `bytes` long: grown (never shrunk) when a call needs more, counted in
// bytes(), freed by adj_rcv_release.  The stream has to be idle (every entry waits for it before it returns).
void* adj_rcv_stage(AdjTapeDev& t, size_t bytes);
// n queries (point, event): d_tt (n, may be null) = interp3d_pt of the event's field at the point, d_grad (3 n, may be null) = G.  d_pts
// (3 n) on the tape's device; shift: subtract the origin of a translated grid first.  d_pts null: the tape's own rows (n ignored)
template <typename T>
void adj_rcv_eval(AdjTapeDev& t, size_t n, const T* d_pts, const int* d_event, bool shift, T* d_tt, T* d_grad);
// d_dtt[r] = the forward chain of d_drcv (4 n_rcv_points) over row r; d_base (n_rows, may be null, may be d_dtt): fl(d_base[r] + that)
template <typename T>
void adj_jvp_rcv(AdjTapeDev& t, const T* d_drcv, const T* d_base, T* d_dtt);
// d_grcv (4 n_rcv_points) = the reverse chains of d_w (n_rows) over the rows of every point
template <typename T>
void adj_vjp_rcv(AdjTapeDev& t, const T* d_w, T* d_grcv);
// ---- moving the receiver points, and the relocation-only system (tests/relocation_reference.py restates both)
// what is wrong with the new receiver points h_pts (3 n_rcv_points values on the host, the caller's coordinates), null: nothing.  A point
// has to be finite and, after the shift of a translated grid, inside the box the solver checks its receivers against.  Host only.
template <typename T>
const char* adj_rcv_move_error(const AdjTapeDev& t, const T* h_pts);
// what the first move adds to the tape
size_t adj_rcv_move_bytes(const AdjTapeDev& t);
// gives every row of receiver point q the receiver h_pts[q] (checked by adj_rcv_move_error): rcv_p, rcv_tt and rcv_G of every row from
// one kernel (one thread per row: shift, interp3d_stencil, interp3d_pt, rcv_grad_pt), the row-order list of the forward mode written by
// the same kernel at the offsets the host formed, the seed list from a stable radix sort of that list by (event, node) and a gather.
// n_seed, the host mirrors (h_rcv_p, h_rw_*) and h_mv_pts follow; a held cotangent is released.  d_pts: the same points on the tape's
// device, or null (h_pts is uploaded through rcv_io).  d_tt (n_rows, may be null) receives rcv_tt.  On the tape's stream; waits for it.
template <typename T>
void adj_rcv_move(AdjTapeDev& t, const T* h_pts, const T* d_pts, T* d_tt);
// d_ge (4 n_rcv_points) = C G^T (op (G C d_ve)), G the operator of adj_jvp_rcv, C = diag(d_scale) (null: none): adj_gn_rjoint without
// its two relaxations -- adj_scale, rcv_rows_kernel, the row operator, rcv_grad_kernel, adj_scale.  d_ve_scaled as in adj_gn_joint.
template <typename T>
void adj_gn_reloc(AdjTapeDev& t, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_ge);
// out = fl(c * in) over n values (in and out may be the same array)
template <typename T>
void adj_scale(AdjTapeDev& t, const T* d_c, const T* d_in, T* d_out, size_t n);
// the receiver joint tangent: adj_jvp of d_ds, then the receiver rows added; outputs as adj_jvp
template <typename T>
int adj_jvp_rjoint(AdjTapeDev& t, const T* d_ds, const T* d_drcv, T* d_dtt, T* d_dfields, int schedule);
// adj_gn_joint with the receiver block in the place of the source block: one tangent relaxation, one adjoint relaxation, the row kernels
template <typename T>
void adj_gn_rjoint(AdjTapeDev& t, const T* d_vs, const T* d_ve, const T* d_scale, T* d_ve_scaled, const RowOp<T>& op, T* d_gs, T* d_ge,
                   int schedule, int* passes_jvp, int* passes_vjp);

// ---- grid-search hypocentre location on the tape's fields (tests/locate_reference.py restates it; kernels in
// fsm_locate.hip).  Where a call's arrays live in loc_work, all on the tape's device: the picks by hypocentre (CSR: off n_hypo + 1, then
// field, time, weight per pick; sw[q] = the sum of q's weights from +0 in ascending pick order, formed by the caller), gx partial minima
// per hypocentre and the three results
struct LocWork {
    int* off = nullptr;
    int* field = nullptr;
    double* sw = nullptr;
    double* time = nullptr;
    double* weight = nullptr;
    double* part_phi = nullptr;
    long long* part_node = nullptr;
    long long* node = nullptr;
    double* t0 = nullptr;
    double* misfit = nullptr;
    int gx = 0;
};
// nodes of a node tile and hypocentres of a chunk of the search kernel on this tape, and whether the tile's field values are staged in LDS
// (they are read from global memory when not even one node per lane fits)
void adj_loc_shape(const AdjTapeDev& t, int* node_tile, int* hypo_chunk, int* staged);
// grows loc_work to what a call with n_hypo hypocentres, n_picks picks and a box of n_box nodes needs and names its parts; grows loc_vol
// to `count` doubles.  Both count in bytes(); AdjDeviceError naming the byte count if an allocation fails.  The stream has to be idle.
LocWork adj_loc_prepare(AdjTapeDev& t, size_t n_hypo, size_t n_picks, long long n_box);
double* adj_loc_volume(AdjTapeDev& t, size_t count);
void adj_loc_release(AdjTapeDev& t);
// the search over box = (i0, i1, j0, j1, k0, k1), half-open node ranges inside the grid, with the picks uploaded to w: fills w.node, w.t0
// and w.misfit (n_hypo each); d_vol (n_hypo x box nodes, x fastest within the box; may be null) receives phi of every box node
template <typename T>
void adj_loc_search(AdjTapeDev& t, const LocWork& w, size_t n_hypo, const int* box, double* d_vol);

}  // namespace ttcr_amd
