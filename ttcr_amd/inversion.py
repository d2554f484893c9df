"""Host-side helpers of the ttcrpy grid classes that inversion codes call next to `raytrace`: interpolation weights of velocity data points
(`compute_D`), smoothing operators (`compute_K`), straight-ray data kernels (`data_kernel_straight_rays`).  They build scipy sparse
matrices from the grid geometry alone -- no solver, no device -- and follow the parameter order of the reference's wrapper
(src/ttcrpy/rgrid.pyx: parameters in C order of `shape`, i.e. z fastest).  Restated with array arithmetic, not ported loop by loop:

  interp_matrix        rgrid.pyx:610-677 (3-D), :3565-3627 (2-D)     one weight 1 per point (cell slowness) or the 2^d multilinear weights
  smoothing_matrices   rgrid.pyx:679-756 (3-D, second differences), :3630-3733 (2-D, order 1 or 2)   one-sided stencils on the faces
  straight_ray_kernel  rgrid.pyx:1381-1720 (3-D), :4259-4470 (2-D, optional elliptical-anisotropy form)   segment lengths per cell

One helper does use a device, through a field tape it is handed: gauss_newton_step, the right-hand side and the solve of a regularised
Gauss-Newton step (FieldTape.solve_normal); no reference counterpart.  And locate, the hypocentres a relocation or a joint
step starts from: the tape's grid search, an off-node start and a Geiger refinement around FieldTape.receiver_eval.
double_difference_step is gauss_newton_step's sibling for differences of two rows (FieldTape.set_row_pairs).
"""
import numpy as np


def _sp():
    import scipy.sparse as sp
    return sp


def interp_matrix(axes, coord, cell_slowness):
    """D (npts x nparams) with D @ params = the parameter field at `coord`.  axes: node coordinates per dimension (uniform spacing).
    Cell slowness: the cell that holds the point.  Node slowness: multilinear weights of the 2^d nodes around it; the cell index is
    int(1e-6 + (c - x0) / dx) as in the reference, clamped so that points on the upper faces take the last cell (the reference indexes
    one node past the end there)."""
    sp = _sp()
    coord = np.asarray(coord, dtype=np.float64)
    nd = len(axes)
    if coord.ndim != 2 or coord.shape[1] != nd:
        raise ValueError('coord should be npts by {0:d}'.format(nd))
    npts = coord.shape[0]
    nn = [a.size for a in axes]
    h = [float(a[1] - a[0]) for a in axes]
    if cell_slowness:
        idx = [np.minimum(((coord[:, d] - axes[d][0]) / h[d]).astype(np.int64), nn[d] - 2) for d in range(nd)]
        col = idx[0]
        for d in range(1, nd):
            col = col * (nn[d] - 1) + idx[d]
        ncell = int(np.prod([n - 1 for n in nn]))
        return sp.csr_matrix((np.ones(npts), (np.arange(npts), col)), shape=(npts, ncell))
    lo = [np.clip((1.e-6 + (coord[:, d] - axes[d][0]) / h[d]).astype(np.int64), 0, nn[d] - 2) for d in range(nd)]
    rows, cols, vals = [], [], []
    for corner in range(1 << nd):
        col = np.zeros(npts, dtype=np.int64)
        w = np.ones(npts)
        for d in range(nd):
            i = lo[d] + ((corner >> (nd - 1 - d)) & 1)          # (i1, i2) outermost along x, like the reference's loops
            col = col * nn[d] + i
            w = w * (1. - np.abs(coord[:, d] - axes[d][i]) / h[d])
        rows.append(np.arange(npts)); cols.append(col); vals.append(w)
    rows = np.stack(rows, axis=1).ravel(); cols = np.stack(cols, axis=1).ravel(); vals = np.stack(vals, axis=1).ravel()
    return sp.csr_matrix((vals, (rows, cols)), shape=(npts, int(np.prod(nn))))


def _stencil_1d(n, h, order):
    """n x n operator along one axis: order 2 -- (1, -2, 1) / h^2 centred, the same stencil shifted inwards on the two end rows;
    order 1 -- (-1/2, 1/2) / h centred, (-1, 1) / h one-sided on the end rows."""
    sp = _sp()
    r = np.arange(n)
    if order == 2:
        if n < 3:
            raise ValueError('second-order smoothing needs at least 3 parameters along every axis')
        c = np.clip(r, 1, n - 2)
        rows = np.repeat(r, 3)
        cols = np.stack((c - 1, c, c + 1), axis=1).ravel()
        vals = np.tile(np.array([1., -2., 1.]) / (h * h), n)
    elif order == 1:
        if n < 2:
            raise ValueError('first-order smoothing needs at least 2 parameters along every axis')
        a = np.maximum(r - 1, 0); b = np.minimum(r + 1, n - 1)
        w = np.where((r == 0) | (r == n - 1), 1.0, 0.5) / h
        rows = np.repeat(r, 2)
        cols = np.stack((a, b), axis=1).ravel()
        vals = np.stack((-w, w), axis=1).ravel()
    else:
        raise ValueError('order value not valid (1 or 2 accepted)')
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def smoothing_matrices(shape, spacings, order=2):
    """One derivative operator per axis acting on the parameters in C order of `shape`: K_d = I x ... x S_d x ... x I."""
    sp = _sp()
    out = []
    for d in range(len(shape)):
        m = None
        for e in range(len(shape)):
            f = _stencil_1d(shape[e], spacings[e], order) if e == d else sp.identity(shape[e], format='csr')
            m = f if m is None else sp.kron(m, f, format='csr')
        out.append(m.tocsr())
    return tuple(out)


def gauss_newton_step(tape, residual, model, row_weight=None, smooth=0., damp=0., **solve_args):
    """The model update of one damped, smoothed Gauss-Newton step on a field tape (rgrid.FieldTape): the right-hand side
        b = tape.vjp(row_weight * residual) - smooth * tape.smooth(model)            (= J^T W r - smooth R s)
    and then tape.solve_normal(b, row_weight=row_weight, smooth=smooth, damp=damp, **solve_args), whose result is returned as it is.
    residual: one value per data row (rcv order); model: the current model vector (n_cols values; not read for smooth == 0).  Host
    glue only: the products are formed where residual and model live, in their dtype; smooth_weights of solve_args shapes R on both
    sides."""
    w = residual if row_weight is None else row_weight * residual
    b = tape.vjp(w)
    if smooth != 0:
        b = b - smooth * tape.smooth(model, solve_args.get('smooth_weights', (1., 1., 1.)))
    return tape.solve_normal(b, row_weight=row_weight, smooth=smooth, damp=damp, **solve_args)


def apply_model_update(tape, slowness, dm):
    """The node slowness after a step dm (n_cols values) on a model tape (raytrace_adjoint(..., wrt='model')):
    slowness + tape.prolong(dm), in slowness's flat node order (x fastest).  The slowness need not be P of anything: the tape
    linearises at whatever was solved and the step moves it by P dm."""
    return slowness + tape.prolong(dm)


def joint_gauss_newton_step(tape, residual, model, row_weight=None, smooth=0., damp=0., source_damp=0., source_scale=None, **solve_args):
    """The update (x, x_src) of slowness and source points of one regularised joint hypocentre-velocity Gauss-Newton step on a field
    tape: the right-hand sides
        b, b_src = tape.vjp(row_weight * residual, return_source_grad=True);   b -= smooth * tape.smooth(model)
    and then tape.solve_joint(b, b_src, row_weight=row_weight, smooth=smooth, damp=damp, source_damp=source_damp,
    source_scale=source_scale, **solve_args), whose result is returned as it is (b_src goes in unscaled: the solver scales it).
    Arguments as gauss_newton_step.  Host glue only."""
    w = residual if row_weight is None else row_weight * residual
    b, b_src = tape.vjp(w, return_source_grad=True)
    if smooth != 0:
        b = b - smooth * tape.smooth(model, solve_args.get('smooth_weights', (1., 1., 1.)))
    return tape.solve_joint(b, b_src, row_weight=row_weight, smooth=smooth, damp=damp, source_damp=source_damp, source_scale=source_scale,
                            **solve_args)


def reciprocal_gauss_newton_step(tape, residual, model, row_weight=None, smooth=0., damp=0., rcv_damp=0., rcv_scale=None, **solve_args):
    """The update (x, x_rcv) of slowness and receiver points of one regularised joint Gauss-Newton step on a field tape in the
    reciprocal layout -- solved from the stations, the hypocentres being the receiver points of the call
    (tape.set_receiver_points) --: the right-hand sides
        b, b_rcv = tape.vjp(row_weight * residual, return_receiver_grad=True);   b -= smooth * tape.smooth(model)
    and then tape.solve_receiver_joint(b, b_rcv, row_weight=row_weight, smooth=smooth, damp=damp, rcv_damp=rcv_damp,
    rcv_scale=rcv_scale, **solve_args), whose result is returned as it is (b_rcv goes in unscaled: the solver scales it).
    Arguments as joint_gauss_newton_step.  Host glue only."""
    w = residual if row_weight is None else row_weight * residual
    b, b_rcv = tape.vjp(w, return_receiver_grad=True)
    if smooth != 0:
        b = b - smooth * tape.smooth(model, solve_args.get('smooth_weights', (1., 1., 1.)))
    return tape.solve_receiver_joint(b, b_rcv, row_weight=row_weight, smooth=smooth, damp=damp, rcv_damp=rcv_damp, rcv_scale=rcv_scale,
                                     **solve_args)


def double_difference_step(tape, residual, pair_residual, model, system='model', row_weight=None, pair_weight=None, smooth=0., damp=0.,
                           block_damp=0., block_scale=None, **solve_args):
    """One regularised Gauss-Newton step on double-difference data (hypoDD / tomoDD style) on a field tape whose row
    pairs are set (tape.set_row_pairs): the weighted rows
        w = row_weight * residual + tape.pair_adjoint(pair_weight * pair_residual)
    (pair_weight=None: ones; residual=None: no absolute data and an all-zero row_weight), the right-hand sides from tape.vjp(w, ...)
    -- with the source gradient for system='joint', the receiver gradient for system='receiver_joint' --, b -= smooth *
    tape.smooth(model), and then the matching solve with pair_weight: tape.solve_normal ('model'), tape.solve_joint ('joint';
    block_damp / block_scale are its source_damp / source_scale) or tape.solve_receiver_joint ('receiver_joint'; rcv_damp / rcv_scale),
    whose result is returned as it is.  residual: one value per data row (rcv order); pair_residual: one value per row pair, the
    observed minus the computed difference.  A common origin-time shift is invisible to pure double-difference data: give block_damp
    > 0 on t0 then.  Host glue only."""
    solves = {'model': None, 'joint': ('solve_joint', 'return_source_grad', 'source'),
              'receiver_joint': ('solve_receiver_joint', 'return_receiver_grad', 'rcv')}
    if system not in solves:
        raise ValueError("system should be 'model', 'joint' or 'receiver_joint', got %r" % (system,))
    if pair_weight is None:
        torch_like = hasattr(pair_residual, 'new_ones')
        pair_weight = pair_residual.new_ones(pair_residual.shape) if torch_like else np.ones(tape.n_pairs, dtype=tape.dtype)
    w = tape.pair_adjoint(pair_weight * pair_residual)
    if residual is None:
        row_weight = w.new_zeros(w.shape) if hasattr(w, 'new_zeros') else np.zeros_like(w)
    else:
        w = w + (residual if row_weight is None else row_weight * residual)
    if solves[system] is None:
        b = tape.vjp(w)
    else:
        b, b_blk = tape.vjp(w, **{solves[system][1]: True})
    if smooth != 0:
        b = b - smooth * tape.smooth(model, solve_args.get('smooth_weights', (1., 1., 1.)))
    if solves[system] is None:
        return tape.solve_normal(b, row_weight=row_weight, pair_weight=pair_weight, smooth=smooth, damp=damp, **solve_args)
    name, _, setting = solves[system]
    return getattr(tape, name)(b, b_blk, row_weight=row_weight, pair_weight=pair_weight, smooth=smooth, damp=damp,
                               **{setting + '_damp': block_damp, setting + '_scale': block_scale}, **solve_args)


# ---- hypocentre location on a field tape in the reciprocal layout
LOCATE_HALVINGS = 4      # halvings of a Geiger step that does not decrease the misfit before the hypocentre stops
LOCATE_MIN_STEP = 1e-6   # ... and it stops when no coordinate of the step exceeds this fraction of dx


def _sum_by_hypo(n_hypo, hyp, ranks, vals):
    """sum of vals (one row per pick) over the picks of every hypocentre, from +0 in ascending pick order: ranks[r] are the picks that
    are the r-th of their hypocentre, so every addition of a pass goes to a different hypocentre"""
    acc = np.zeros((n_hypo,) + vals.shape[1:])
    for sel in ranks:
        acc[hyp[sel]] = acc[hyp[sel]] + vals[sel]
    return acc


def _misfit(n_hypo, hyp, ranks, sw, tm, wt, tt):
    """(t0, phi) per hypocentre by locate_grid's formula with tt (one row per pick; further axes: alternatives) in the place of the node
    values; hypocentres with sw == 0 get NaN"""
    ex = (slice(None),) + (None,) * (tt.ndim - 1)
    r = tm[ex] - tt
    with np.errstate(invalid='ignore', divide='ignore'):
        t0 = _sum_by_hypo(n_hypo, hyp, ranks, wt[ex] * r) / sw[(slice(None),) + (None,) * (tt.ndim - 1)]
    d = r - t0[hyp]
    return t0, _sum_by_hypo(n_hypo, hyp, ranks, wt[ex] * (d * d))


def _geiger_step(n_hypo, hyp, ranks, sw, tm, wt, tt, G, damp):
    """The damped Gauss-Newton step of every hypocentre from the rows (1, Gx, Gy, Gz) and residuals tm - tt of its picks: the origin
    time is eliminated (weighted means taken off the residuals and the gradients), the 3 x 3 system A dx = b with A = sum w Gc Gc^T +
    damp * (trace / 3) I, b = sum w Gc rc is solved through the adjugate, elementwise.  Returns (dx (n_hypo, 3), ok): ok is False where
    the determinant is not a positive finite number (the step is zero there)."""
    r = tm - tt
    with np.errstate(invalid='ignore', divide='ignore'):
        rbar = _sum_by_hypo(n_hypo, hyp, ranks, wt * r) / sw
        Gbar = _sum_by_hypo(n_hypo, hyp, ranks, wt[:, None] * G) / sw[:, None]
    rc, Gc = r - rbar[hyp], G - Gbar[hyp]
    wG = wt[:, None] * Gc
    b = _sum_by_hypo(n_hypo, hyp, ranks, wG * rc[:, None])
    a = {}
    for i in range(3):
        for j in range(i, 3):
            a[i, j] = _sum_by_hypo(n_hypo, hyp, ranks, wG[:, i] * Gc[:, j])
    lam = damp * ((a[0, 0] + a[1, 1] + a[2, 2]) / 3.0)
    a00, a11, a22, a01, a02, a12 = a[0, 0] + lam, a[1, 1] + lam, a[2, 2] + lam, a[0, 1], a[0, 2], a[1, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11   # the adjugate of a symmetric matrix
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    ok = np.isfinite(det) & (det > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        dx = np.stack([c00 * b[:, 0] + c01 * b[:, 1] + c02 * b[:, 2], c01 * b[:, 0] + c11 * b[:, 1] + c12 * b[:, 2],
                       c02 * b[:, 0] + c12 * b[:, 1] + c22 * b[:, 2]], axis=1) / det[:, None]
    ok &= np.all(np.isfinite(dx), axis=1)
    dx[~ok] = 0.0
    return dx, ok


def locate(tape, pick_hypo, pick_field, pick_time, pick_weight=None, n_hypo=None, box=None, refine=10, damp=1e-3):
    """Hypocentres from picks on a field tape in the reciprocal layout (field e: the traveltimes from station e): the grid search
    tape.locate_grid, a start off the grid planes, and up to `refine` Geiger iterations around tape.receiver_eval.  Picks, weights,
    n_hypo and box as locate_grid takes them (ValueError alike).  Returns (t0, xyz, misfit, info): t0 (n_hypo,), xyz (n_hypo, 3) user
    coordinates and misfit (n_hypo,), float64 numpy arrays -- the misfit is locate_grid's phi with the interpolated traveltime in the place
    of the node value; a hypocentre the grid search gives no node (-1) gets NaN coordinates, t0 0 and misfit 0 and is left alone.  xyz can go
    straight to raytrace_adjoint(..., rcv=xyz) and set_receiver_points.  Plain numpy in float64 on the host; the device is used by
    locate_grid and receiver_eval only.
      1. The grid search.
      2. The start: of the up to 8 cells that touch the best node, the centres of those inside the grid and inside the box (an axis on
         which the box holds a single node plane restricts nothing) are candidates; one receiver_eval call evaluates all of them, the
         smallest misfit wins, the first in the order x outer, z inner, minus before plus among equal ones.  A point on a grid plane
         has a zero gradient along that axis, a node along all three: a cell centre has none.
      3. The refinement, one receiver_eval call per iteration for the hypocentres still moving.  From traveltimes and gradients at its
         point a hypocentre forms the Geiger step (rows (1, Gx, Gy, Gz), weights w, origin time eliminated, A = sum w Gc Gc^T + damp *
         (trace / 3) I, solved through the 3 x 3 adjugate) and proposes point + step, every coordinate clipped to the grid.  An
         iteration evaluates the proposals: where the misfit is smaller than at the point, the proposal becomes the point (a counted
         iteration) and a new full step is formed there; otherwise the same step is proposed halved once more, and after
         LOCATE_HALVINGS halvings without a decrease the hypocentre stops.  It also stops when the system is singular or no
         coordinate of a step exceeds LOCATE_MIN_STEP * dx.  The misfit therefore never increases; refine=0 returns the start.
    info: node, grid_t0 and grid_misfit (the grid search's results), start_xyz and start_misfit (step 2), iterations (accepted steps
    per hypocentre) and misfit (the final one, as returned)."""
    from .rgrid import FieldTape

    if not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError('refine should be an integer >= 0, got %r' % (refine,))
    nn3, dx, origin = tape.geometry
    nq, off, fld, tm, wt, b6 = FieldTape.locate_csr(tape.n_events, nn3, pick_hypo, pick_field, pick_time, pick_weight, n_hypo, box)
    node, t0g, phig = tape.locate_grid(pick_hypo, pick_field, pick_time, pick_weight, n_hypo=nq, box=box)
    node = np.asarray(node, dtype=np.int64)
    wt = np.ones(tm.shape[0]) if wt is None else wt
    hyp = np.repeat(np.arange(nq), np.diff(off))
    live = node >= 0
    keep = live[hyp]                                     # the picks of the hypocentres that have a node
    hyp, fld, tm, wt = hyp[keep], fld[keep], tm[keep], wt[keep]
    rank = np.arange(keep.size)[keep] - off[:-1][hyp] if hyp.size else hyp
    ranks = [np.flatnonzero(rank == r) for r in range(int(rank.max()) + 1 if rank.size else 0)]
    sw = _sum_by_hypo(nq, hyp, ranks, wt)
    nn = np.asarray(nn3, dtype=np.int64)
    lo, hi = origin, origin + (nn - 1) * dx

    def evaluate(pts):
        """traveltime and gradient of every kept pick at the point of its hypocentre, float64"""
        tt, G = tape.receiver_eval(pts[hyp], fld, return_grad=True)
        return np.asarray(tt, dtype=np.float64), np.asarray(G, dtype=np.float64)

    # 2. the start
    ijk = np.stack([node % nn[0], (node // nn[0]) % nn[1], node // (nn[0] * nn[1])], axis=1)
    ijk[~live] = 0
    blo = np.array([b6[0], b6[2], b6[4]], dtype=np.int64)
    bhi = np.array([b6[1], b6[3], b6[5]], dtype=np.int64) - 1     # last node of the box
    single = bhi == blo
    clo, chi = np.where(single, 0, blo), np.where(single, nn - 2, bhi - 1)   # lower nodes of the cells allowed
    cand = np.zeros((nq, 8, 3))
    valid = np.zeros((nq, 8), dtype=bool)
    c = 0
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                cell = ijk + (np.array([sx, sy, sz]) - 1) // 2                      # lower node of the cell on that side
                valid[:, c] = np.all((cell >= clo) & (cell <= chi), axis=1) & live
                cand[:, c] = origin + (np.where(valid[:, c, None], cell, np.clip(cell, 0, nn - 2)) + 0.5) * dx
                c += 1
    n_pick = hyp.shape[0]
    if n_pick:
        tt8, G8 = tape.receiver_eval(cand[hyp].reshape(-1, 3), np.repeat(fld, 8), return_grad=True)
        tt8 = np.asarray(tt8, dtype=np.float64).reshape(n_pick, 8)
        G8 = np.asarray(G8, dtype=np.float64).reshape(n_pick, 8, 3)
    else:
        tt8, G8 = np.zeros((0, 8)), np.zeros((0, 8, 3))
    t08, phi8 = _misfit(nq, hyp, ranks, sw, tm, wt, tt8)
    phi8 = np.where(valid & ~np.isnan(phi8), phi8, np.inf)
    best = np.argmin(phi8, axis=1)                        # (the first among equal ones)
    rows = np.arange(nq)
    x = cand[rows, best]
    phi, t0 = phi8[rows, best], t08[rows, best]
    live &= np.isfinite(phi)
    x[~live], phi[~live], t0[~live] = np.nan, 0.0, 0.0
    start_xyz, start_phi = x.copy(), phi.copy()
    iterations = np.zeros(nq, dtype=np.int64)

    # 3. the refinement
    moving = live.copy()
    halvings = np.zeros(nq, dtype=np.int64)
    step = np.zeros((nq, 3))
    if refine > 0 and n_pick:
        step, ok = _geiger_step(nq, hyp, ranks, sw, tm, wt, tt8[np.arange(n_pick), best[hyp]], G8[np.arange(n_pick), best[hyp]], damp)
        moving &= ok & (np.max(np.abs(step), axis=1) > LOCATE_MIN_STEP * dx)
    for _ in range(int(refine)):
        if not moving.any():
            break
        trial = np.where(moving[:, None], np.clip(x + step * (0.5 ** halvings)[:, None], lo, hi), x)
        sel = moving[hyp]                                   # only the picks of the hypocentres still moving are evaluated
        tt, G = np.zeros(n_pick), np.zeros((n_pick, 3))
        tt[sel], G[sel] = [np.asarray(a, dtype=np.float64) for a in tape.receiver_eval(trial[hyp[sel]], fld[sel], return_grad=True)]
        t0t, phit = _misfit(nq, hyp, ranks, sw, tm, wt, tt)
        better = moving & (phit < phi)
        x[better], phi[better], t0[better] = trial[better], phit[better], t0t[better]
        iterations[better] += 1
        halvings[better] = 0
        new_step, ok = _geiger_step(nq, hyp, ranks, sw, tm, wt, tt, G, damp)
        step[better] = new_step[better]
        worse = moving & ~better
        halvings[worse] += 1
        moving &= np.where(better, ok & (np.max(np.abs(step), axis=1) > LOCATE_MIN_STEP * dx), halvings <= LOCATE_HALVINGS)
    info = dict(node=node, grid_t0=np.asarray(t0g, dtype=np.float64), grid_misfit=np.asarray(phig, dtype=np.float64), start_xyz=start_xyz,
                start_misfit=start_phi, iterations=iterations, misfit=phi.copy())
    return t0, x, phi, info


# ---- relocation on a fixed model, on a field tape in the reciprocal layout
def relocation_step(tape, residual, pair_residual=None, row_weight=None, pair_weight=None, rcv_damp=0., rcv_scale=None, **solve_args):
    """One relocation-only Gauss-Newton step on a field tape: the sibling of double_difference_step without the slowness block.  The
    weighted rows
        w = row_weight * residual + tape.pair_adjoint(pair_weight * pair_residual)
    (row_weight=None: ones; pair_residual=None: no pairs; pair_weight=None: ones; residual=None: no absolute data and an all-zero
    row_weight), the right-hand side rhs_rcv = tape.vjp_receiver(w) -- no relaxation --, and tape.solve_receiver with the same weights,
    whose result (x_rcv, or (x_rcv, info) with return_info=True) is returned as it is: (dt0, dx, dy, dz) per receiver point.  Host glue
    only; arrays stay where they are (numpy or torch)."""
    w = None
    if pair_residual is not None:
        if pair_weight is None:
            torch_like = hasattr(pair_residual, 'new_ones')
            pair_weight = pair_residual.new_ones(pair_residual.shape) if torch_like else np.ones(tape.n_pairs, dtype=tape.dtype)
        w = tape.pair_adjoint(pair_weight * pair_residual)
    if residual is None:
        if w is None:
            raise ValueError('residual and pair_residual are both None: no data')
        row_weight = w.new_zeros(w.shape) if hasattr(w, 'new_zeros') else np.zeros_like(w)
    else:
        rows = residual if row_weight is None else row_weight * residual
        w = rows if w is None else w + rows
    return tape.solve_receiver(tape.vjp_receiver(w), row_weight=row_weight, rcv_damp=rcv_damp, rcv_scale=rcv_scale,
                               pair_weight=pair_weight if pair_residual is not None else None, **solve_args)


def relocate(tape, t_obs, t0, row_weight=None, pair_dt=None, pair_weight=None, n_iter=10, rcv_damp=1e-3, rcv_scale=None, maxiter=20,
             rtol=1e-6):
    """Relocate the receiver points of a field tape on a fixed model -- the hypocentres of a reciprocal layout, absolute times and
    (with pair_dt) double-difference times together, hypoDD proper --, with no solve and no relaxation: the loop runs on
    tape.move_receiver_points, tape.vjp_receiver and tape.solve_receiver.
      t_obs: the observed arrival time of every data row (rcv order); t0: the origin time of every receiver point, (n_rcv_points,);
      row_weight: a weight per data row or None (ones); pair_dt: the observed difference of every row pair (tape.set_row_pairs) or
      None (no pairs); pair_weight: a weight per pair or None (ones); rcv_damp, rcv_scale, maxiter, rtol: solve_receiver's.
    It starts from tape.receiver_points() (a point without rows that was never moved sits at the grid's lower corner).  Per iteration:
    the residuals r = t_obs - (tt + t0[point]) and r_p = pair_dt - Q (tt + t0[point]) from the tape's current traveltimes, one
    relocation_step, and the proposal (t0 + f d_t0, xyz + f d_xyz) with f = 1, every coordinate clipped to the grid, applied by
    move_receiver_points.  It is accepted if the total weighted misfit sum(row_weight r^2) + sum(pair_weight r_p^2) did not rise;
    otherwise the same step is tried with f halved, LOCATE_HALVINGS times at most, after which the points are moved back and the
    loop ends.  Everything is in the tape's dtype except the misfit, which is summed in float64.  Returns (t0, xyz, misfit_history, info):
    the misfit at the start and after every accepted iteration (it never rises); info holds iterations (accepted), halvings (per
    accepted iteration) and cg (the info dict of every solve).  The tape is left at the returned points, ready for the next
    solve_receiver_joint.  With torch tensors on the tape's device nothing but the scalar misfits crosses to the host."""
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError('n_iter should be an integer >= 0, got %r' % (n_iter,))
    on_dev = type(t_obs).__module__.startswith('torch') and t_obs.device.type == 'cuda'
    dt = np.dtype(tape.dtype)
    nn3, dx, origin = tape.geometry
    lo = np.asarray(origin, dtype=dt)
    hi = lo + (np.asarray(nn3) - 1).astype(dt) * dt.type(dx)
    por = np.asarray(tape.rcv_point_of_row, dtype=np.int64)
    if por.size and por.min() < 0:
        raise ValueError('relocate needs every data row on the tape')
    xyz = tape.receiver_points()
    xyz = np.where(np.isnan(xyz), lo, xyz).astype(dt)
    if on_dev:
        import torch

        tdt = torch.float32 if dt == np.float32 else torch.float64
        as_t = lambda a: None if a is None else torch.as_tensor(a, device=t_obs.device).to(tdt)   # noqa: E731
        lo, hi, xyz, por = as_t(lo), as_t(hi), as_t(xyz), torch.as_tensor(por, device=t_obs.device)
        clip = lambda a: torch.minimum(torch.maximum(a, lo), hi)   # noqa: E731
        total = lambda a: float(a.double().sum())   # noqa: E731
    else:
        as_t = lambda a: None if a is None else np.asarray(a.detach().cpu().numpy() if hasattr(a, 'detach') else a, dtype=dt)   # noqa: E731
        clip = lambda a: np.minimum(np.maximum(a, lo), hi)   # noqa: E731
        total = lambda a: float(np.sum(np.asarray(a, dtype=np.float64)))   # noqa: E731
    t_obs, t0, row_weight, pair_dt, pair_weight = as_t(t_obs), as_t(t0), as_t(row_weight), as_t(pair_dt), as_t(pair_weight)
    if tuple(t0.shape) != (tape.n_rcv_points,):
        raise ValueError('t0 should hold %d values (one per receiver point), got shape %s' % (tape.n_rcv_points, tuple(t0.shape)))

    def residuals(tt, t0_):
        tc = tt + t0_[por]
        r = t_obs - tc
        rp = pair_dt - tape.pair_difference(tc) if pair_dt is not None else None
        m = total((r * r) if row_weight is None else (row_weight * (r * r)))
        if rp is not None:
            m = m + total((rp * rp) if pair_weight is None else (pair_weight * (rp * rp)))
        return r, rp, m

    tt = tape.move_receiver_points(xyz)
    r, rp, m = residuals(tt, t0)
    history, halvings, cg = [m], [], []
    for _ in range(int(n_iter)):
        d, info = relocation_step(tape, r, rp, row_weight, pair_weight, rcv_damp=rcv_damp, rcv_scale=rcv_scale, maxiter=maxiter, rtol=rtol,
                                  return_info=True)
        cg.append(info)
        accepted = False
        for h in range(LOCATE_HALVINGS + 1):
            f = 0.5 ** h   # (a power of two: exact in either dtype)
            t0_new, xyz_new = t0 + f * d[:, 0], clip(xyz + f * d[:, 1:])
            r_new, rp_new, m_new = residuals(tape.move_receiver_points(xyz_new), t0_new)
            if m_new <= m:
                t0, xyz, r, rp, m, accepted = t0_new, xyz_new, r_new, rp_new, m_new, True
                history.append(m)
                halvings.append(h)
                break
        if not accepted:
            tape.move_receiver_points(xyz)
            break
    return t0, xyz, history, dict(iterations=len(halvings), halvings=halvings, cg=cg)


def straight_ray_kernel(Tx, Rx, axes, aniso=False):
    """L (nrays x ncells) with L @ slowness = traveltimes along the straight segments Tx[n] -> Rx[n] through the cells of the grid `axes`
    (node coordinates per dimension, any spacing).  Cells in C order ((ix * ncy + iy) * ncz + iz).  aniso (2-D only): L is nrays x 2 ncells,
    the x components of the segments in the first block and the z components in the second (signed, with the ray oriented towards
    increasing x -- increasing z for a vertical ray -- as the reference walks it)."""
    sp = _sp()
    Tx = np.asarray(Tx, dtype=np.float64); Rx = np.asarray(Rx, dtype=np.float64)
    nd = len(axes)
    if Tx.shape != Rx.shape or Tx.ndim != 2 or Tx.shape[1] != nd:
        raise ValueError('Tx and Rx should be nrays by {0:d}, one row per source-receiver pair'.format(nd))
    if aniso and nd != 2:
        raise ValueError('aniso: 2-D grids only')
    axes = [np.asarray(a, dtype=np.float64) for a in axes]
    nc = [a.size - 1 for a in axes]
    ncell = int(np.prod(nc))
    data, indices, indptr = [], [], [0]
    for n in range(Tx.shape[0]):
        p1, p2 = Tx[n], Rx[n]
        if p1[0] > p2[0] or (p1[0] == p2[0] and p1[-1] > p2[-1]):
            p1, p2 = p2, p1
        v = p2 - p1
        d = float(np.sqrt(np.sum(v * v)))
        if d == 0.0:
            indptr.append(len(data))
            continue
        ts = [np.array([0.0, 1.0])]
        for a in range(nd):
            if v[a] != 0.0:
                t = (axes[a] - p1[a]) / v[a]
                ts.append(t[(t > 0.0) & (t < 1.0)])
        t = np.unique(np.concatenate(ts))
        dt = np.diff(t)
        keep = dt > 1.e-14
        tm = 0.5 * (t[:-1] + t[1:])[keep]
        dt = dt[keep]
        cell = np.zeros(tm.size, dtype=np.int64)
        for a in range(nd):
            ia = np.clip(np.searchsorted(axes[a], p1[a] + tm * v[a], side='right') - 1, 0, nc[a] - 1)
            cell = cell * nc[a] + ia
        if not aniso:
            data.extend((dt * d).tolist()); indices.extend(cell.tolist())
        else:
            for c, s in zip(cell.tolist(), dt.tolist()):
                indices.append(c); data.append(s * v[0])
                indices.append(c + ncell); data.append(s * v[1])
        indptr.append(len(data))
    return sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int64), np.array(indptr, dtype=np.int64)),
                         shape=(Tx.shape[0], 2 * ncell if aniso else ncell))
