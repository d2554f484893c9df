"""The double-difference rows of the field tape restated in numpy, in the tape's dtype, every operation rounded on its
own: the data operator B = diag(rw) + Q^T diag(pw) Q, row p of Q holding +1 at row a_p and -1 at row b_p, and the products and solves
that apply it between their tangent and adjoint halves, composed from the restatements of 6c to 6k (which stay as they are).  Rows are
tape rows throughout.  The entries of row r are the pairs p with a_p == r (sign +) or b_p == r (sign -), in ascending p."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_reference as JR  # noqa: E402
import receiver_reference as RR  # noqa: E402


def check_pairs(n_rows, a, b):
    """the checks of ttcr_fsm_dd_pairs: ValueError naming the first offending pair"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError('row_a and row_b should hold one row per pair each')
    if a.size >= 2 ** 30:
        raise ValueError('at most 2^30 - 1 row pairs')
    for p in range(a.size):
        if a[p] == b[p]:
            raise ValueError('pair %d joins a row to itself' % p)
        if not (0 <= a[p] < n_rows and 0 <= b[p] < n_rows):
            raise ValueError('pair %d names a row outside 0 .. n_rows - 1' % p)
    return a, b


def csr(n_rows, a, b):
    """(off, ent): the entries of every row, one int 2 p + sign each (sign 1: the row is subtracted), ascending p within a row"""
    a, b = check_pairs(n_rows, a, b)
    cnt = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(cnt, a + 1, 1)
    np.add.at(cnt, b + 1, 1)
    off = np.cumsum(cnt)
    ent = np.zeros(2 * a.size, dtype=np.int64)
    fill = off[:-1].copy()
    for p in range(a.size):
        ent[fill[a[p]]] = 2 * p
        fill[a[p]] += 1
        ent[fill[b[p]]] = 2 * p + 1
        fill[b[p]] += 1
    return off, ent


def pair_difference(x, a, b):
    """Q x: d[p] = fl(x[a_p] - x[b_p])"""
    x = np.asarray(x)
    dt = x.dtype
    with np.errstate(all='ignore'):
        return (x[np.asarray(a, dtype=np.int64)] - x[np.asarray(b, dtype=np.int64)]).astype(dt)


def _chains(start, u, n_rows, a, b):
    dt = u.dtype
    off, ent = csr(n_rows, a, b)
    out = np.array(start, dtype=dt, copy=True)
    with np.errstate(all='ignore'):
        for r in range(n_rows):
            acc = out[r]
            for c in range(off[r], off[r + 1]):
                p, sign = divmod(int(ent[c]), 2)
                acc = dt.type(acc - u[p]) if sign else dt.type(acc + u[p])
            out[r] = acc
    return out


def pair_adjoint(y, n_rows, a, b):
    """Q^T y: per row a chain from +0 over its entries, acc = fl(acc + y[p]) for sign + and fl(acc - y[p]) for sign -"""
    y = np.asarray(y)
    return _chains(np.zeros(n_rows, dtype=y.dtype), y, n_rows, a, b)


def row_operator(x, a, b, row_weight=None, pair_weight=None):
    """B x: u[p] = fl(pw[p] * d[p]) (pair_weight None: d[p]); out[r] = a chain from fl(rw[r] * x[r]) (row_weight None: from x[r]) over
    the entries of r, acc = fl(acc +- u[p])"""
    x = np.asarray(x)
    dt = x.dtype
    d = pair_difference(x, a, b)
    with np.errstate(all='ignore'):
        u = d if pair_weight is None else (np.asarray(pair_weight, dtype=dt) * d).astype(dt)
        start = x if row_weight is None else (np.asarray(row_weight, dtype=dt) * x).astype(dt)
    return _chains(start, u, x.shape[0], a, b)


def dense_operator(n_rows, a, b, row_weight=None, pair_weight=None):
    """diag(rw) + Q^T diag(pw) Q as a dense float64 matrix"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    Q = np.zeros((a.size, n_rows))
    Q[np.arange(a.size), a] = 1.0
    Q[np.arange(a.size), b] = -1.0
    rw = np.ones(n_rows) if row_weight is None else np.asarray(row_weight, dtype=np.float64)
    pw = np.ones(a.size) if pair_weight is None else np.asarray(pair_weight, dtype=np.float64)
    return np.diag(rw) + Q.T @ (pw[:, None] * Q)


def row_bound(x, a, b, row_weight=None, pair_weight=None):
    """per row (deg_r + 3) u sum |terms| of B x: the forward-error bound of the chain (every term carries at most two roundings of its
    own -- the difference and the product -- and the chain deg_r more)"""
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.shape[0]
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    rw = np.ones(n) if row_weight is None else np.asarray(row_weight, dtype=np.float64)
    pw = np.ones(a.size) if pair_weight is None else np.asarray(pair_weight, dtype=np.float64)
    t = np.abs(pw * (x64[a] - x64[b]))   # (a difference of two values of the dtype carries one relative rounding of its own)
    mag = np.abs(rw * x64)
    deg = np.zeros(n)
    np.add.at(mag, a, t)
    np.add.at(mag, b, t)
    np.add.at(deg, a, 1)
    np.add.at(deg, b, 1)
    return (deg + 3) * np.finfo(np.asarray(x).dtype).eps / 2 * mag


# ---- the products: today's product with its fl(row_weight * dtt) step replaced by row_operator(dtt, row_weight, pair_weight)
def gauss_newton(jvp, vjp, v, a, b, row_weight=None, pair_weight=None):
    """vjp(row_operator(jvp(v))): jvp(v) -> rows and vjp(w) -> model gradient are restated, dense or the device's own calls"""
    return vjp(row_operator(jvp(v), a, b, row_weight, pair_weight))


def joint_product(jvp_joint, vjp_source, v, v_src, a, b, dtype, row_weight=None, pair_weight=None, source_scale=None):
    """(g, g_src) of gauss_newton_joint with pairs: jvp_joint(v, ve) -> rows, vjp_source(w) -> (g, gsrc), the scale handling of 6j"""
    dt = np.dtype(dtype)
    ve = JR.scale_block(source_scale, v_src, dt)
    w = row_operator(np.asarray(jvp_joint(v, ve), dtype=dt), a, b, row_weight, pair_weight)
    g, gsrc = vjp_source(w)
    return g, JR.scale_block(source_scale, gsrc, dt)


def receiver_joint_product(jvp, vjp, G, point_of_row, n_points, v, v_rcv, a, b, row_weight=None, pair_weight=None, rcv_scale=None):
    """(g, g_rcv) of gauss_newton_receiver_joint with pairs: 6k's joint tangent, w = row_operator(dtt), vjp(w) and the receiver
    gradient of w, the scale handling of 6k"""
    dt = np.dtype(G.dtype)
    ve = JR.scale_block(rcv_scale, v_rcv, dt)
    dtt = RR.joint_tangent(jvp(v), G, point_of_row, ve)
    w = row_operator(dtt, a, b, row_weight, pair_weight)
    return vjp(w), JR.scale_block(rcv_scale, RR.reverse(G, point_of_row, n_points, w), dt)
