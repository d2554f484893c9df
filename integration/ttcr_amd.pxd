# integration/ttcr_amd.pxd -- Cython declarations of the C ABI (include/ttcr_amd.h); the two adapter classes a ttcrpy
# maintainer adds to src/ttcrpy/rgrid.pxd are in ttcr_amd_adapters.pxd (they need the reference headers).  tests/test_integration.py cythonizes a module that cimports this file
# (Cython 3 is in the image), so the stub is checked by the compiler, not by eye.
from libc.stdint cimport uint32_t
from libcpp cimport bool
from libcpp.vector cimport vector

cdef extern from "ttcr_amd.h" nogil:
    ctypedef struct ttcr_fsm_grid:
        pass
    cdef enum:
        TTCR_F32
        TTCR_F64
    cdef enum:
        TTCR_OK
        TTCR_ERR_VALUE
        TTCR_ERR_RUNTIME
        TTCR_ERR_DEVICE
        TTCR_ERR_UNSUPPORTED
    ctypedef struct ttcr_fsm_timing:
        double sweep_ms
        double total_ms
        long long kernel_launches
        long long node_updates
        long long evaluated_updates
        int iterations
        int n_sources
    int ttcr_fsm_device_count()
    const char* ttcr_fsm_last_error()
    int ttcr_fsm3d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncy, uint32_t ncz,
                          double dx, double xmin, double ymin, double zmin, double eps, int maxit, int weno, int n_slots,
                          int translate_origin, int device)
    int ttcr_fsm2d_create(ttcr_fsm_grid** out, int dtype, int cell_slowness, uint32_t ncx, uint32_t ncz, double dx, double dz,
                          double xmin, double zmin, double eps, int maxit, int weno, int rotated_template, int n_slots,
                          int device)
    void ttcr_fsm_destroy(ttcr_fsm_grid* g)
    int ttcr_fsm_set_slowness(ttcr_fsm_grid* g, const void* s, size_t n)
    int ttcr_fsm_set_slowness_device(ttcr_fsm_grid* g, const void* d_s, size_t n)
    int ttcr_fsm_set_slowness_c_order(ttcr_fsm_grid* g, const void* s, size_t n)
    int ttcr_fsm_get_slowness(ttcr_fsm_grid* g, void* out, size_t n)
    int ttcr_fsm_raytrace(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                          void* tt_out)
    int ttcr_fsm_raytrace_multi(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0,
                                const int* rx_off, const void* rx, void* tt_out)
    int ttcr_fsm_get_tt(ttcr_fsm_grid* g, int slot, void* out, size_t n)
    int ttcr_fsm_get_tt_device(ttcr_fsm_grid* g, int slot, void** d_ptr)
    int ttcr_fsm_get_tt_device_view(ttcr_fsm_grid* g, int slot, void** d_ptr, size_t* stride)
    int ttcr_fsm_interp(ttcr_fsm_grid* g, int slot, int n_pts, const void* pts, void* tt_out)
    int ttcr_fsm_compute_slowness(ttcr_fsm_grid* g, int n_pts, const void* pts, int translated, void* out)
    int ttcr_fsm_get_niter(ttcr_fsm_grid* g, int slot, int* niter, int* niterw)
    int ttcr_fsm_n_slots(const ttcr_fsm_grid* g)
    size_t ttcr_fsm_n_nodes(const ttcr_fsm_grid* g)
    size_t ttcr_fsm_n_cells(const ttcr_fsm_grid* g)
    int ttcr_fsm_set_option(ttcr_fsm_grid* g, const char* key, double value)
    int ttcr_fsm_rays_size(const ttcr_fsm_grid* g, size_t* n_rays, size_t* n_points)
    int ttcr_fsm_get_rays(const ttcr_fsm_grid* g, long long* offsets, void* pts)
    # per-slot rays and the matrices M / L (the r_data, m_data and l_data overloads of Grid3D / Grid2D::raytrace)
    int ttcr_fsm_raytrace_rays(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                               void* tt_out)
    int ttcr_fsm_slot_rays_size(const ttcr_fsm_grid* g, int slot, size_t* n_rays, size_t* n_points)
    int ttcr_fsm_get_slot_rays(const ttcr_fsm_grid* g, int slot, long long* offsets, void* pts)
    int ttcr_fsm_raytrace_m(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                            void* tt_out)
    int ttcr_fsm_raytrace_rm(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                             void* tt_out)
    int ttcr_fsm_raytrace_multi_m(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                  const void* rx, void* tt_out, int with_rays)
    int ttcr_fsm_multi_m_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz)
    int ttcr_fsm_get_multi_m(const ttcr_fsm_grid* g, long long* row_off, long long* j, void* v)
    # the field tape: exact discrete adjoint of the first-order 3-D node solver (adjoint-state gradient)
    ctypedef struct ttcr_fsm_adjoint:
        pass
    int ttcr_fsm_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0,
                                        const int* rx_off, const void* rx, void* tt_out, ttcr_fsm_adjoint** tape)
    # the same for a 3-D cell grid: the model vector of vjp / jvp / gn then holds n_cells values (ttcr_fsm_adjoint_model tells which)
    int ttcr_fsm_raytrace_multi_adjoint_cells(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0,
                                              const int* rx_off, const void* rx, void* tt_out, ttcr_fsm_adjoint** tape)
    int ttcr_fsm_adjoint_model(const ttcr_fsm_adjoint* t, int* cells, size_t* n_params, size_t* n_nodes)
    # the same for a coarse model grid under a 3-D node grid (DESIGN.md 6n): the model vector holds mx my mz values; P and P^T on a tape or a grid
    int ttcr_fsm_model_raytrace_multi_adjoint(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0,
                                              const int* rx_off, const void* rx, void* tt_out, ttcr_fsm_adjoint** tape, const int* model_shape)
    int ttcr_fsm_model_shape(const ttcr_fsm_adjoint* t, int* is_model, int* shape)
    int ttcr_fsm_model_tape_prolong(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device)
    int ttcr_fsm_model_tape_restrict(const ttcr_fsm_adjoint* t, const void* g, int g_on_device, void* out, int out_on_device)
    int ttcr_fsm_model_device(const ttcr_fsm_grid* g, int* device)
    int ttcr_fsm_model_prolong(ttcr_fsm_grid* g, const int* model_shape, const void* v, int v_on_device, void* out, int out_on_device)
    int ttcr_fsm_model_restrict(ttcr_fsm_grid* g, const int* model_shape, const void* gr, int g_on_device, void* out, int out_on_device)
    int ttcr_fsm_adjoint_size(const ttcr_fsm_adjoint* t, size_t* n_events, size_t* n_rows, size_t* n_nodes)
    int ttcr_fsm_adjoint_bytes(const ttcr_fsm_adjoint* t, size_t* bytes)
    int ttcr_fsm_adjoint_device(const ttcr_fsm_adjoint* t, int* device)
    int ttcr_fsm_adjoint_get_field(const ttcr_fsm_adjoint* t, size_t event, void* out)
    int ttcr_fsm_adjoint_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device,
                             void* grad, int grad_on_device, int schedule, int* passes)
    # forward mode of the same linearisation: J v (receiver rows and / or fields) and the Gauss-Newton product J^T (row_weight * J v)
    int ttcr_fsm_adjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, void* dtt, int dtt_on_device,
                             void* dfields, int df_on_device, int schedule, int* passes)
    int ttcr_fsm_adjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device,
                            void* out, int out_on_device, int schedule, int* passes_jvp, int* passes_vjp)
    int ttcr_fsm_adjoint_points(const ttcr_fsm_adjoint* t, size_t* n_points, int* event_of_point)
    int ttcr_fsm_adjoint_jvp_source(const ttcr_fsm_adjoint* t, const void* dsrc, int dsrc_on_device, int n_cols, void* dtt,
                                    int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes)
    int ttcr_fsm_adjoint_vjp_source(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device,
                                    void* grad, int grad_on_device, void* gsrc, int gsrc_on_device, int schedule, int* passes)
    # second-order products: hold keeps lam of a cotangent on the tape, hvp is the derivative of its vjp in a direction, newton adds J^T W J v
    int ttcr_fsm_adjoint_hold(ttcr_fsm_adjoint* t, const void* w, int w_on_device, const void* field_cot, int fc_on_device, void* grad,
                              int grad_on_device, int schedule, int* passes)
    int ttcr_fsm_adjoint_release(ttcr_fsm_adjoint* t)
    int ttcr_fsm_adjoint_hvp(ttcr_fsm_adjoint* t, const void* v, int v_on_device, void* out, int out_on_device, int schedule,
                             int* passes_jvp, int* passes_vjp)
    int ttcr_fsm_adjoint_newton(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* row_weight, int rw_on_device,
                                void* out, int out_on_device, int schedule, int* passes_jvp, int* passes_vjp)
    # block products: n_cols model vectors per call, relaxed in groups of four; column k has the bits of the one-column call
    int ttcr_fsm_adjoint_jvp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* ds, int ds_on_device, void* dtt, int dtt_on_device,
                                   void* dfields, int df_on_device, int schedule, int* passes)
    int ttcr_fsm_adjoint_vjp_block(const ttcr_fsm_adjoint* t, int n_cols, const void* w, int w_on_device, void* grad, int grad_on_device,
                                   int schedule, int* passes)
    int ttcr_fsm_adjoint_gn_block(const ttcr_fsm_adjoint* t, int n_cols, const void* v, int v_on_device, const void* row_weight,
                                  int rw_cols, int rw_on_device, void* out, int out_on_device, int schedule, int* passes_jvp,
                                  int* passes_vjp)
    int ttcr_fsm_adjoint_block_release(ttcr_fsm_adjoint* t)
    int ttcr_fsm_adjoint_free(ttcr_fsm_adjoint* t)
    # normal equations of a field tape: smoothing operator, fixed-order inner product, CG around the Gauss-Newton / Newton product
    int ttcr_fsm_normal_tile_edge(int dtype)
    int ttcr_fsm_normal_smooth(ttcr_fsm_adjoint* t, const void* v, int v_on_device, const double* weights, void* out, int out_on_device)
    int ttcr_fsm_normal_dot(ttcr_fsm_adjoint* t, const void* a, int a_on_device, const void* b, int b_on_device, double* result)
    int ttcr_fsm_normal_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* row_weight, int rw_on_device,
                              double smooth, const double* smooth_weights, double damp, const void* x0, int x0_on_device, int maxiter,
                              double rtol, int newton, int schedule, void* x, int x_on_device, int* status, int* iterations, double* rho,
                              double* pq, int* passes)
    int ttcr_fsm_normal_release(ttcr_fsm_adjoint* t)
    # joint hypocentre-velocity system of a field tape: one relaxation for both operands, the joint product, CG on the joint system
    int ttcr_fsm_joint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* dsrc, int dsrc_on_device, void* dtt,
                           int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes)
    int ttcr_fsm_joint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_src, int vs_on_device,
                          const void* row_weight, int rw_on_device, const double* source_scale, void* out, int out_on_device,
                          void* out_src, int os_on_device, int schedule, int* passes_jvp, int* passes_vjp)
    int ttcr_fsm_joint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_src, int rs_on_device,
                             const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                             const double* source_damp, const double* source_scale, int maxiter, double rtol, int schedule, void* x,
                             int x_on_device, void* x_src, int xs_on_device, int* status, int* iterations, double* rho, double* pq,
                             int* passes)
    int ttcr_fsm_joint_release(ttcr_fsm_adjoint* t)
    # receiver-point derivatives of a field tape and the joint system with the receiver block (the reciprocal layout)
    int ttcr_fsm_rcv_eval(const ttcr_fsm_adjoint* t, size_t n_pts, const void* pts, int pts_on_device, const int* event_of_pt,
                                  void* tt, int tt_on_device, void* grad, int grad_on_device)
    int ttcr_fsm_rcv_points(ttcr_fsm_adjoint* t, const int* set_point_of_row, size_t set_n_points, size_t* n_points,
                            int* point_of_row, int* differing_rows)
    int ttcr_fsm_rcv_jvp(const ttcr_fsm_adjoint* t, const void* drcv, int drcv_on_device, void* dtt, int dtt_on_device)
    int ttcr_fsm_rcv_vjp(const ttcr_fsm_adjoint* t, const void* w, int w_on_device, void* grcv, int grcv_on_device)
    int ttcr_fsm_rjoint_jvp(const ttcr_fsm_adjoint* t, const void* ds, int ds_on_device, const void* drcv, int drcv_on_device, void* dtt,
                            int dtt_on_device, void* dfields, int df_on_device, int schedule, int* passes)
    int ttcr_fsm_rjoint_gn(const ttcr_fsm_adjoint* t, const void* v, int v_on_device, const void* v_rcv, int vr_on_device,
                           const void* row_weight, int rw_on_device, const double* rcv_scale, void* out, int out_on_device,
                           void* out_rcv, int or_on_device, int schedule, int* passes_jvp, int* passes_vjp)
    int ttcr_fsm_rjoint_solve(ttcr_fsm_adjoint* t, const void* rhs, int rhs_on_device, const void* rhs_rcv, int rr_on_device,
                              const void* row_weight, int rw_on_device, double smooth, const double* smooth_weights, double damp,
                              const double* rcv_damp, const double* rcv_scale, int maxiter, double rtol, int schedule, void* x,
                              int x_on_device, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq,
                              int* passes)
    int ttcr_fsm_rcv_release(ttcr_fsm_adjoint* t)
    # grid-search hypocentre location on the fields of a field tape
    int ttcr_fsm_loc_geometry(const ttcr_fsm_adjoint* t, int* nn, double* dx, double* origin)
    int ttcr_fsm_loc_shape(const ttcr_fsm_adjoint* t, int* node_tile, int* hypo_chunk, int* staged)
    int ttcr_fsm_loc_grid(const ttcr_fsm_adjoint* t, size_t n_hypo, const long long* hypo_off, const int* pick_field,
                          const double* pick_time, const double* pick_weight, const int* box, long long* node_out, double* t0_out,
                          double* misfit_out, void* volume_out, int volume_on_device)
    int ttcr_fsm_loc_release(ttcr_fsm_adjoint* t)
    # double-difference rows of a field tape
    int ttcr_fsm_dd_pairs(ttcr_fsm_adjoint* t, const int* set_row_a, const int* set_row_b, size_t set_n_pairs, size_t* n_pairs,
                          int* row_a, int* row_b, long long* bad_pair)
    int ttcr_fsm_dd_apply(const ttcr_fsm_adjoint* t, int mode, const void* x, int x_on_device, const void* row_weight, int rw_on_device,
                          const void* pair_weight, int pw_on_device, void* out, int out_on_device)
    int ttcr_fsm_dd_gn(const ttcr_fsm_adjoint* t, int system, int newton, const void* v, int v_on_device, const void* v_b,
                       int vb_on_device, const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device,
                       const double* b_scale, void* out, int out_on_device, void* out_b, int ob_on_device, int schedule,
                       int* passes_jvp, int* passes_vjp)
    int ttcr_fsm_dd_solve(ttcr_fsm_adjoint* t, int system, const void* rhs, int rhs_on_device, const void* rhs_b, int rb_on_device,
                          const void* row_weight, int rw_on_device, const void* pair_weight, int pw_on_device, double smooth,
                          const double* smooth_weights, double damp, const double* b_damp, const double* b_scale, const void* x0,
                          int x0_on_device, int maxiter, double rtol, int newton, int schedule, void* x, int x_on_device, void* x_b,
                          int xb_on_device, int* status, int* iterations, double* rho, double* pq, int* passes)
    int ttcr_fsm_dd_release(ttcr_fsm_adjoint* t)
    # moving the receiver points of a field tape, and the relocation-only system
    int ttcr_fsm_reloc_move(ttcr_fsm_adjoint* t, const void* pts, int pts_on_device, void* tt, int tt_on_device)
    int ttcr_fsm_reloc_get_points(const ttcr_fsm_adjoint* t, double* pts)
    int ttcr_fsm_reloc_gn(const ttcr_fsm_adjoint* t, const void* v_rcv, int vr_on_device, const void* row_weight, int rw_on_device,
                          const void* pair_weight, int pw_on_device, const double* rcv_scale, void* out_rcv, int or_on_device)
    int ttcr_fsm_reloc_solve(ttcr_fsm_adjoint* t, const void* rhs_rcv, int rr_on_device, const void* row_weight, int rw_on_device,
                             const void* pair_weight, int pw_on_device, const double* rcv_damp, const double* rcv_scale, int maxiter,
                             double rtol, void* x_rcv, int xr_on_device, int* status, int* iterations, double* rho, double* pq)
    int ttcr_fsm_slot_m_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz)
    int ttcr_fsm_get_slot_m(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* j, void* v)
    int ttcr_fsm_raytrace_l(ttcr_fsm_grid* g, int slot, int n_tx, const void* tx, const void* t0, int n_rx, const void* rx,
                            void* tt_out, int with_rays)
    int ttcr_fsm_raytrace_multi_l(ttcr_fsm_grid* g, int n_src, const int* tx_off, const void* tx, const void* t0, const int* rx_off,
                                  const void* rx, void* tt_out, int with_rays)
    int ttcr_fsm_multi_l_size(const ttcr_fsm_grid* g, size_t* n_rows, size_t* nnz)
    int ttcr_fsm_get_multi_l(const ttcr_fsm_grid* g, long long* row_off, long long* cell, void* v)
    int ttcr_fsm_slot_l_size(const ttcr_fsm_grid* g, int slot, size_t* n_rows, size_t* nnz)
    int ttcr_fsm_get_slot_l(const ttcr_fsm_grid* g, int slot, long long* row_off, long long* cell, void* v)
    int ttcr_fsm_last_timing(const ttcr_fsm_grid* g, ttcr_fsm_timing* out)
    int ttcr_fsm_unit_order(int dim, int dtype, int stage, int by_time, uint32_t nnx, uint32_t nny, uint32_t nnz, uint32_t* out,
                            size_t capacity, size_t* n_units)
    int ttcr_fsm_sweep_plan(int dim, int dtype, int weno, uint32_t nnx, uint32_t nny, uint32_t nnz, int n_slots, const char* const* keys,
                            const double* values, int n_options, int wg_cap, int stage, int batch, int layout, char* name, size_t name_len,
                            long long* out)
    const char* ttcr_fsm_build_id()
