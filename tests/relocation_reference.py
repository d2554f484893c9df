"""Numpy restatement of what DESIGN.md 6o adds to the field tape: a move of the receiver points (the row quantities a moved tape holds),
the relocation-only Gauss-Newton product C G^T B G C, conjugate gradients on it, and the relocation loop of inversion.relocate.  The device
side is rcv_move_kernel and the sort behind it (ttcr_amd/csrc/fsm_adjoint.hip), adj_gn_reloc and the fourth system of adj_solve
(fsm_normal.hip).  Everything is computed in the dtype asked for, every product, difference, quotient and sum rounded on its own, in the
order of the definition; the misfit alone is summed in float64.

Conventions as in receiver_reference: rows in tape row order, a receiver block is (n_points, 4) = (t0, x, y, z) per receiver point,
point_of_row maps rows to points.  A Layout describes a tape: its fields, the grid (nn3, dx, the lower corner `origin` in user coordinates,
`translate`: the grid subtracts its origin from every point first), the event and the point of every row, and the row pairs."""
import numpy as np

import dd_reference as DD
import joint_reference as JR
import receiver_reference as RR

LOCATE_HALVINGS = 4   # inversion.LOCATE_HALVINGS, restated


class Layout:
    def __init__(self, fields, nn3, dx, origin, event_of_row, point_of_row, n_points, translate=False, pairs=None):
        self.fields = [np.asarray(f).ravel() for f in fields]
        self.dtype = np.dtype(self.fields[0].dtype)
        self.nn3, self.dx = tuple(int(n) for n in nn3), float(dx)
        self.origin = np.asarray(origin, dtype=self.dtype)
        self.translate = bool(translate)
        self.event_of_row = np.asarray(event_of_row, dtype=np.int64)
        self.point_of_row = np.asarray(point_of_row, dtype=np.int64)
        self.n_points = int(n_points)
        self.pairs = None if pairs is None else (np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64))

    @property
    def bounds(self):
        """(lo, hi) per axis in the grid dtype: the box a moved point is clipped to and checked against"""
        dt = self.dtype
        return self.origin, (self.origin + (np.asarray(self.nn3) - 1).astype(dt) * dt.type(self.dx)).astype(dt)

    def solver_points(self, xyz):
        """the points as the solver sees them, and the origin it interpolates with"""
        dt = self.dtype
        xyz = np.asarray(xyz, dtype=dt).reshape(-1, 3)
        if self.translate:
            return (xyz - self.origin).astype(dt), np.zeros(3, dtype=dt)
        return xyz, self.origin


def check_move(layout, xyz):
    """the checks of move_receiver_points: shape, finite, inside the grid"""
    a = np.asarray(xyz)
    if a.shape != (layout.n_points, 3) or a.dtype.kind not in 'fiu':
        raise ValueError('xyz should be (%d, 3) real numbers' % layout.n_points)
    a = a.astype(layout.dtype)
    if not np.isfinite(a).all():
        raise ValueError('xyz should be finite')
    lo, hi = layout.bounds
    if a.size and ((a < lo) | (a > hi)).any():
        raise ValueError('Receiver outside grid')
    return a


def move(layout, xyz):
    """(tt, G, p) of every row after a move to xyz (n_points, 3) user coordinates: the receiver of row r is xyz[point_of_row[r]], p is that
    point as the solver sees it, tt and G are receiver_reference.evaluate's on the field of the row's event"""
    ps, mn = layout.solver_points(check_move(layout, xyz))
    p = ps[layout.point_of_row]
    tt, G = RR.evaluate_points(layout.fields, layout.nn3, layout.dx, mn, p, layout.event_of_row)
    return tt, G, p


def row_operator(layout, x, row_weight=None, pair_weight=None):
    """B x: the diagonal alone without pair_weight, dd_reference.row_operator with it"""
    dt = layout.dtype
    x = np.asarray(x, dtype=dt)
    if pair_weight is None:
        return x if row_weight is None else (np.asarray(row_weight, dtype=dt) * x).astype(dt)
    a, b = layout.pairs
    return DD.row_operator(x, a, b, row_weight, pair_weight)


def product(layout, G, v_rcv, row_weight=None, rcv_scale=None, pair_weight=None):
    """gauss_newton_receiver: C G^T B (G C v_rcv) -- scale, the forward chain of every row, the row operator, the reverse chains of every
    point, scale"""
    dt = layout.dtype
    ve = JR.scale_block(rcv_scale, v_rcv, dt)
    w = row_operator(layout, RR.forward(G, layout.point_of_row, ve), row_weight, pair_weight)
    return JR.scale_block(rcv_scale, RR.reverse(G, layout.point_of_row, layout.n_points, w), dt)


def dense(layout, G, row_weight=None, rcv_scale=None, pair_weight=None):
    """the matrix of `product` in float64, (4 n_points, 4 n_points): C Gm^T B Gm C with Gm the dense (n_rows, 4 n_points) operator"""
    n = len(G)
    Gm = np.zeros((n, 4 * layout.n_points))
    for r in range(n):
        q = layout.point_of_row[r]
        Gm[r, 4 * q] = 1.0
        Gm[r, 4 * q + 1:4 * q + 4] = np.asarray(G[r], dtype=np.float64)
    rw = np.ones(n) if row_weight is None else np.asarray(row_weight, dtype=np.float64)
    B = np.diag(rw)
    if pair_weight is not None:
        a, b = layout.pairs
        B = DD.dense_operator(n, a, b, row_weight, pair_weight)
    c = np.ones(4 * layout.n_points) if rcv_scale is None else np.broadcast_to(np.asarray(rcv_scale, dtype=np.float64), (layout.n_points, 4)).ravel()
    return c[:, None] * (Gm.T @ B @ Gm) * c[None, :], Gm, B


def cg(prod, rhs_rcv, dtype, rcv_damp=None, rcv_scale=None, maxiter=20, rtol=1e-6):
    """solve_receiver: joint_reference.cg's recurrence on a vector whose model block is empty -- the block alone, n_joint = 4 n_points.
    prod(p_rcv) returns the product with the column scaling already inside.  Returns (x_rcv, info)."""
    dt = np.dtype(dtype)
    none = np.zeros(0, dtype=dt)
    _, x, info = JR.cg(lambda ps, pe: (none, prod(pe)), none, rhs_rcv, dt, source_damp=rcv_damp, source_scale=rcv_scale, maxiter=maxiter,
                       rtol=rtol)
    return x, info


def step(layout, G, residual, pair_residual=None, row_weight=None, pair_weight=None, rcv_damp=0., rcv_scale=None, maxiter=20, rtol=1e-6):
    """inversion.relocation_step: w = Q^T (pw * r_p) + rw * r, rhs = G^T w, then cg"""
    dt = layout.dtype
    w = None
    if pair_residual is not None:
        a, b = layout.pairs
        if pair_weight is None:
            pair_weight = np.ones(len(a), dtype=dt)
        w = DD.pair_adjoint((np.asarray(pair_weight, dtype=dt) * np.asarray(pair_residual, dtype=dt)).astype(dt), len(G), a, b)
    rows = np.asarray(residual, dtype=dt) if row_weight is None else (np.asarray(row_weight, dtype=dt) * np.asarray(residual, dtype=dt)).astype(dt)
    w = rows if w is None else (w + rows).astype(dt)
    rhs = RR.reverse(G, layout.point_of_row, layout.n_points, w)
    pw = pair_weight if pair_residual is not None else None
    return cg(lambda p: product(layout, G, p, row_weight, rcv_scale, pw), rhs, dt, rcv_damp=rcv_damp, rcv_scale=rcv_scale, maxiter=maxiter,
              rtol=rtol)


def relocate(layout, xyz, t_obs, t0, row_weight=None, pair_dt=None, pair_weight=None, n_iter=10, rcv_damp=1e-3, rcv_scale=None, maxiter=20,
             rtol=1e-6):
    """inversion.relocate from the points xyz: (t0, xyz, misfit_history, info)"""
    dt = layout.dtype
    cast = lambda a: None if a is None else np.asarray(a, dtype=dt)   # noqa: E731
    t_obs, t0, row_weight, pair_dt, pair_weight = cast(t_obs), cast(t0), cast(row_weight), cast(pair_dt), cast(pair_weight)
    lo, hi = layout.bounds
    por = layout.point_of_row

    def total(a):
        return float(np.sum(np.asarray(a, dtype=np.float64)))

    def residuals(tt, t0_):
        tc = (tt + t0_[por]).astype(dt)
        r = (t_obs - tc).astype(dt)
        m = total((r * r).astype(dt) if row_weight is None else (row_weight * (r * r).astype(dt)).astype(dt))
        rp = None
        if pair_dt is not None:
            rp = (pair_dt - DD.pair_difference(tc, *layout.pairs)).astype(dt)
            m = m + total((rp * rp).astype(dt) if pair_weight is None else (pair_weight * (rp * rp).astype(dt)).astype(dt))
        return r, rp, m

    xyz = np.asarray(xyz, dtype=dt).reshape(-1, 3)
    tt, G, _ = move(layout, xyz)
    r, rp, m = residuals(tt, t0)
    history, halvings, infos = [m], [], []
    for _ in range(n_iter):
        d, info = step(layout, G, r, rp, row_weight, pair_weight, rcv_damp, rcv_scale, maxiter, rtol)
        infos.append(info)
        accepted = False
        for h in range(LOCATE_HALVINGS + 1):
            f = dt.type(0.5 ** h)
            t0_new = (t0 + (f * d[:, 0]).astype(dt)).astype(dt)
            xyz_new = np.minimum(np.maximum((xyz + (f * d[:, 1:]).astype(dt)).astype(dt), lo), hi)
            tt_new, G_new, _ = move(layout, xyz_new)
            r_new, rp_new, m_new = residuals(tt_new, t0_new)
            if m_new <= m:
                t0, xyz, G, r, rp, m, accepted = t0_new, xyz_new, G_new, r_new, rp_new, m_new, True
                history.append(m)
                halvings.append(h)
                break
        if not accepted:
            break
    return t0, xyz, history, dict(iterations=len(halvings), halvings=halvings, cg=infos)


class StandInTape:
    """The methods inversion.relocate and inversion.relocation_step call on a FieldTape, on a Layout: no device."""

    def __init__(self, layout, xyz):
        self.layout = layout
        self.dtype = layout.dtype
        self.n_rcv_points = layout.n_points
        self.rcv_point_of_row = layout.point_of_row.copy()
        self.n_pairs = 0 if layout.pairs is None else len(layout.pairs[0])
        self.geometry = (layout.nn3, layout.dx, np.asarray(layout.origin, dtype=np.float64))
        self.moves = 0
        self.move_receiver_points(xyz)
        self.moves = 0

    def move_receiver_points(self, xyz):
        tt, G, _ = move(self.layout, xyz)
        self.xyz, self.G = np.array(xyz, dtype=self.dtype), G
        self.moves += 1
        return tt

    def receiver_points(self):
        return self.xyz.copy()

    def vjp_receiver(self, w):
        return RR.reverse(self.G, self.layout.point_of_row, self.layout.n_points, np.asarray(w, dtype=self.dtype))

    def pair_difference(self, x):
        return DD.pair_difference(np.asarray(x, dtype=self.dtype), *self.layout.pairs)

    def pair_adjoint(self, y):
        return DD.pair_adjoint(np.asarray(y, dtype=self.dtype), len(self.G), *self.layout.pairs)

    def gauss_newton_receiver(self, v_rcv, row_weight=None, rcv_scale=None, pair_weight=None):
        return product(self.layout, self.G, v_rcv, row_weight, rcv_scale, pair_weight)

    def solve_receiver(self, rhs_rcv, row_weight=None, rcv_damp=0.0, rcv_scale=None, maxiter=20, rtol=1e-6, return_info=False,
                       pair_weight=None):
        x, info = cg(lambda p: product(self.layout, self.G, p, row_weight, rcv_scale, pair_weight), rhs_rcv, self.dtype, rcv_damp=rcv_damp,
                     rcv_scale=rcv_scale, maxiter=maxiter, rtol=rtol)
        return (x, info) if return_info else x
