"""Numpy restatement of the field tape's receiver-point derivatives and of the receiver joint system (the device side is
rcv_eval_kernel, rcv_rows_kernel and rcv_grad_kernel of ttcr_amd/csrc/fsm_adjoint.hip and the joint solver of fsm_normal.hip): the
receiver interpolation as the solver evaluates it, its derivative with respect to the point with the cell and the on-plane flags held
fixed, the forward and reverse chains over receiver points, the receiver joint tangent and product, and conjugate gradients on the
column-scaled joint system.  Everything is computed in the dtype asked for, every product, difference, quotient and sum rounded on its
own, in the order of the definition.

Conventions as in adjoint_reference: node m = (k * nny + j) * nnx + i (x fastest); nn3 = (nnx, nny, nnz); mn = (xmin, ymin, zmin) as the
solver sees them (zeros on a translated grid, whose points arrive with the origin already subtracted); one spacing dx.  A receiver
block is an (n_points, 4) array, (t0, x, y, z) per receiver point; point_of_row maps the rows (tape row order) to points.
"""
import numpy as np

import joint_reference as JR

SMALL2 = 1.e-4 * 1.e-4


def axis_terms(dtype, nn3, dx, mn, p):
    """(lo, on, w1, w2) per axis as interp3d_pt / interp3d_stencil compute them"""
    dt = np.dtype(dtype)
    dx = dt.type(dx)
    lo, on, w1, w2 = [], [], [], []
    for a in range(3):
        pa, ca = dt.type(p[a]), dt.type(mn[a])
        v = SMALL2 + float(dt.type(pa - ca) / dx)
        l = 0 if v < 0 else int(v)
        lo.append(l)
        on.append(float(abs(dt.type(pa - dt.type(ca + dt.type(l) * dx)))) < SMALL2)
        w1.append(dt.type(dt.type(dt.type(ca + dt.type(l + 1) * dx) - pa) / dx))
        w2.append(dt.type(dt.type(pa - dt.type(ca + dt.type(l) * dx)) / dx))
    return lo, on, w1, w2


def _nested(dt, vals, axes, on, w1, w2):
    """interp3d_pt's nested interpolation of `vals`, an array with one axis of length 1 (on) or 2 per entry of `axes` (ascending):
    the highest axis first (z, then y, then x), fl(fl(t1 * w1) + fl(t2 * w2)); an axis the point lies on contributes its one plane"""
    v = np.asarray(vals, dtype=dt)
    for a in reversed(axes):
        if on[a]:
            v = v[..., 0]
        else:
            v = ((v[..., 0] * w1[a]).astype(dt) + (v[..., 1] * w2[a]).astype(dt)).astype(dt)
    return dt.type(v)


def _node(nn3, c):
    return (c[2] * nn3[1] + c[1]) * nn3[0] + c[0]


def evaluate(T, nn3, dx, mn, p):
    """(tt, G) at one point p in the field T: tt with the bits of interp3d_pt, G[a] = d tt / d p_a with the cell and the on flags held
    fixed -- +0 on an axis with on[a], else fl(I_a / dx), I_a the nested interpolation over the remaining axes that are not on of the
    differences fl(T[hi_a] - T[lo_a]); node indices clamped as TT clamps them"""
    T = np.asarray(T).ravel()
    dt = np.dtype(T.dtype)
    lo, on, w1, w2 = axis_terms(dt, nn3, dx, mn, p)
    c = [[min(lo[a], nn3[a] - 1), min(lo[a] + 1, nn3[a] - 1)] for a in range(3)]
    n = [1 if on[a] else 2 for a in range(3)]
    vals = np.zeros((n[0], n[1], n[2]), dtype=dt)
    for ii in range(n[0]):
        for jj in range(n[1]):
            for kk in range(n[2]):
                vals[ii, jj, kk] = T[_node(nn3, (c[0][ii], c[1][jj], c[2][kk]))]
    tt = _nested(dt, vals, [0, 1, 2], on, w1, w2)
    G = np.zeros(3, dtype=dt)
    for a in range(3):
        if on[a]:
            continue
        rest = [b for b in range(3) if b != a]
        d = np.zeros((n[rest[0]], n[rest[1]]), dtype=dt)
        for ib in range(n[rest[0]]):
            for ic in range(n[rest[1]]):
                hi, lw = [0, 0, 0], [0, 0, 0]
                hi[a], lw[a] = c[a][1], c[a][0]
                hi[rest[0]] = lw[rest[0]] = c[rest[0]][ib]
                hi[rest[1]] = lw[rest[1]] = c[rest[1]][ic]
                d[ib, ic] = dt.type(T[_node(nn3, hi)] - T[_node(nn3, lw)])
        G[a] = dt.type(_nested(dt, d, rest, on, w1, w2) / dt.type(dx))
    return tt, G


def evaluate_points(fields, nn3, dx, mn, pts, event_of_pt):
    """(tt (n,), G (n, 3)) of n queries (point, event); pts as the solver sees them"""
    dt = np.dtype(np.asarray(fields[0]).dtype)
    pts = np.asarray(pts, dtype=dt).reshape(-1, 3)
    tt, G = np.zeros(len(pts), dtype=dt), np.zeros((len(pts), 3), dtype=dt)
    for i, p in enumerate(pts):
        tt[i], G[i] = evaluate(fields[int(event_of_pt[i])], nn3, dx, mn, p)
    return tt, G


def check_points(rcv_rows, point_of_row, n_points=None):
    """the checks of set_receiver_points on tape rows: (n_points) or ValueError naming the first offending pair of rows"""
    por = np.asarray(point_of_row)
    top = int(por.max()) + 1 if por.size else 0
    n_points = top if n_points is None else n_points
    if por.size and por.min() < 0 or n_points < top:
        raise ValueError('point index out of range')
    first = {}
    rcv_rows = np.ascontiguousarray(rcv_rows)
    for r, q in enumerate(por):
        f = first.setdefault(int(q), r)
        if rcv_rows[f].tobytes() != rcv_rows[r].tobytes():
            raise ValueError('rows %d and %d share a receiver point but their receiver coordinates differ' % (f, r))
    return n_points


def forward(G, point_of_row, drcv):
    """dtt_rcv[r]: acc = drcv[q][0], then per axis x, y, z acc = fl(acc + fl(G[r][a] * drcv[q][1 + a]))"""
    dt = np.dtype(G.dtype)
    drcv = np.asarray(drcv, dtype=dt).reshape(-1, 4)
    out = np.zeros(len(G), dtype=dt)
    for r in range(len(G)):
        d = drcv[point_of_row[r]]
        acc = d[0]
        for a in range(3):
            acc = dt.type(acc + dt.type(G[r, a] * d[1 + a]))
        out[r] = acc
    return out


def reverse(G, point_of_row, n_points, w):
    """grcv (n_points, 4): over the rows of a point in ascending row order, from +0, acc = fl(acc + w[r]) for t0 and
    acc = fl(acc + fl(w[r] * G[r][a])) for x, y, z; a point without rows keeps +0"""
    dt = np.dtype(G.dtype)
    w = np.asarray(w, dtype=dt)
    g = np.zeros((n_points, 4), dtype=dt)
    for r in range(len(G)):
        q = point_of_row[r]
        g[q, 0] = dt.type(g[q, 0] + w[r])
        for a in range(3):
            g[q, 1 + a] = dt.type(g[q, 1 + a] + dt.type(w[r] * G[r, a]))
    return g


def joint_tangent(jvp_rows, G, point_of_row, drcv):
    """dtt[r] = fl(jvp(ds)[r] + dtt_rcv[r]); jvp_rows = the rows of the slowness tangent (tangent_reference, or the device's jvp)"""
    dt = np.dtype(G.dtype)
    return (np.asarray(jvp_rows, dtype=dt) + forward(G, point_of_row, drcv)).astype(dt)


def joint_product(jvp, vjp, G, point_of_row, n_points, v, v_rcv, row_weight=None, rcv_scale=None):
    """(g, g_rcv) of gauss_newton_receiver_joint: jvp(v) -> rows and vjp(w) -> model gradient are the slowness half (restated, dense, or
    the device's own calls: the product has the bits of vjp(w)); rows in tape row order"""
    dt = np.dtype(G.dtype)
    ve = JR.scale_block(rcv_scale, v_rcv, dt)
    dtt = joint_tangent(jvp(v), G, point_of_row, ve)
    w = dtt if row_weight is None else (np.asarray(row_weight, dtype=dt) * dtt).astype(dt)
    g = vjp(w)
    return g, JR.scale_block(rcv_scale, reverse(G, point_of_row, n_points, w), dt)


def cg(product, rhs, rhs_rcv, dtype, smooth_op=None, smooth=0.0, damp=0.0, rcv_damp=None, rcv_scale=None, maxiter=20, rtol=1e-6):
    """Conjugate gradients from zero on the receiver joint system: 6j's recurrence (joint_reference.cg) with the receiver block in the
    place of the source block.  product(p, p_rcv) returns (g, g_rcv) with the column scaling already inside.  Returns (x, x_rcv, info)."""
    return JR.cg(product, rhs, rhs_rcv, dtype, smooth_op=smooth_op, smooth=smooth, damp=damp, source_damp=rcv_damp, source_scale=rcv_scale,
                 maxiter=maxiter, rtol=rtol)
