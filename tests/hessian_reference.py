"""Numpy restatement of the second-order products of the field tape (the device side is ttcr_amd/csrc/fsm_adjoint.hip):
hvp(v) = d/dv of the adjoint-state gradient for a held cotangent (w, field_cotangent), and newton(v, W) = J^T W J v + hvp(v) from one
adjoint relaxation.  Everything is computed in the dtype asked for, every product, difference, quotient and sum rounded on its own, in
the order of the definition.  Built on adjoint_reference (couplings, seeds, adjoint_event) and tangent_reference (tangent_event, rows).

Per event, lam the adjoint of the held seeds, mu the field tangent of v, u_axis(n) the active upwind neighbour of n:

    dD[n]     = sum over the active axes, order x, y, z, the first term assigned, of fl(mu[n] - mu[u_axis(n)])          n not frozen
    e_axis(n) = fl(fl(fl(mu[n] - mu[u]) - fl(fl(fl(T[n] - T[u]) / D[n]) * dD[n])) / D[n])
    q[j]      = +0, then over the neighbours n that have j as an active upwind neighbour, order x-, x+, y-, y+, z-, z+:
                q[j] = fl(q[j] + fl(lam[n] * e_axis(n)))
    lam2      = the adjoint of the seeds (field cotangent q; for newton also the rows fl(W[r] * (J v)[r]))
    r[m]      = fl(fl(lam[m] * fl(fl(dx * fl(v[m] * dx)) - fl(fl(fl(dx * fl(s[m] * dx)) / D[m]) * dD[m]))) / D[m])     m not frozen
    out_e[m]  = fl(grad_e(lam2)[m] + r[m])   m not frozen;    fl(d_m * lam2[m])   m frozen
    out       = the events summed ascending from +0

Conventions as in adjoint_reference.py.
"""
import numpy as np

import adjoint_reference as AR
import tangent_reference as TR


def second_order_terms(T, s, dx, nn3, frozen, lam, mu, v):
    """(q, r) of one event: the seeds of the second adjoint relaxation and the direct term of the gradient (0 at frozen nodes)"""
    dt = T.dtype
    dx = dt.type(dx)
    nnx, nny, nnz = nn3
    upper, active, D, fz = AR.couplings(T, nn3, frozen)
    stride = (1, nnx, nnx * nny)
    m_all = np.arange(T.size)
    pos = (m_all % nnx, (m_all // nnx) % nny, m_all // (nnx * nny))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        # per axis: u (index of the upwind neighbour, m itself where the axis is inactive), p' and the coupling T[n] - T[u]
        up_idx, dp, dT = [], [], []
        dD = np.zeros(T.size, dtype=dt)
        first = np.ones(T.size, dtype=bool)
        for axis in range(3):
            u = np.where(active[axis], np.where(upper[axis], m_all + stride[axis], m_all - stride[axis]), m_all)
            p = (mu - mu[u]).astype(dt)
            dD = np.where(active[axis], np.where(first, p, (dD + p).astype(dt)), dD)
            first = first & ~active[axis]
            up_idx.append(u)
            dp.append(p)
            dT.append((T - T[u]).astype(dt))
        # e_axis(n) for every node and axis (unused where the axis is inactive)
        e = [(((dp[a] - ((dT[a] / D).astype(dt) * dD).astype(dt)).astype(dt)) / D).astype(dt) for a in range(3)]
    q = np.zeros(T.size, dtype=dt)
    for axis in range(3):
        for side in (0, 1):
            # neighbour n of j on that side (side 0: lower index) has j as its active upwind neighbour
            if side == 0:
                j = m_all[pos[axis] > 0]
                n = j - stride[axis]
                f = active[axis][n] & upper[axis][n]
            else:
                j = m_all[pos[axis] < nn3[axis] - 1]
                n = j + stride[axis]
                f = active[axis][n] & ~upper[axis][n]
            j, n = j[f], n[f]
            q[j] = (q[j] + (lam[n] * e[axis][n]).astype(dt)).astype(dt)
    s = np.asarray(s, dtype=dt).ravel()
    v = np.asarray(v, dtype=dt).ravel()
    cv = (dx * (v * dx).astype(dt)).astype(dt)
    cs = (dx * (s * dx).astype(dt)).astype(dt)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        r = ((lam * (cv - ((cs / D).astype(dt) * dD).astype(dt)).astype(dt)).astype(dt) / D).astype(dt)
    r[fz] = 0
    return q, r, fz


def product_event(T, s, dx, nn3, mn, frozen, rcv, w, field_cot, v, row_weight=None, newton=False, lam=None):
    """out_e, lam, q, r, dtt of one event.  w / field_cot: the held cotangent (either may be None); row_weight (per receiver of the event,
    or None = ones without a product) is used by the Newton product only."""
    dt = T.dtype
    if lam is None:
        lam = AR.adjoint_event(T, s, dx, nn3, frozen, AR.seeds(dt, nn3, dx, mn, rcv, w, field_cot))[0]
    mu = TR.tangent_event(T, s, dx, nn3, frozen, v)
    q, r, fz = second_order_terms(T, s, dx, nn3, frozen, lam, mu, v)
    rows = None
    dtt = None
    if newton:
        dtt = TR.rows(dt, nn3, dx, mn, rcv, mu)
        rows = dtt if row_weight is None else (np.asarray(row_weight, dtype=dt) * dtt).astype(dt)
    g2 = AR.seeds(dt, nn3, dx, mn, rcv, rows, q)
    lam2, grad2 = AR.adjoint_event(T, s, dx, nn3, frozen, g2)
    out = grad2.copy()
    out[~fz] = (grad2[~fz] + r[~fz]).astype(dt)
    return out, lam, q, r, dtt


def _product(fields, s, dx, nn3, mn, sources, v, rcvs, ws, field_cot, row_weights, newton):
    dt = np.dtype(fields[0].dtype)
    s = np.asarray(s, dtype=dt).ravel()
    v = np.asarray(v, dtype=dt).ravel()
    out = np.zeros(s.size, dtype=dt)
    for e, T in enumerate(fields):
        fr = AR.frozen_nodes(dt, nn3, dx, mn, sources[e])
        o = product_event(np.asarray(T, dtype=dt).ravel(), s, dx, nn3, mn, fr, None if rcvs is None else rcvs[e],
                          None if ws is None else ws[e], None if field_cot is None else field_cot[e], v,
                          None if row_weights is None else row_weights[e], newton)[0]
        out = (out + o).astype(dt)
    return out


def hvp(fields, s, dx, nn3, mn, sources, v, rcvs=None, ws=None, field_cot=None):
    """d/dv of AR.adjoint(fields(s), s, ...; ws, field_cot) with the cotangent held fixed: arguments as AR.adjoint, v one value per node"""
    return _product(fields, s, dx, nn3, mn, sources, v, rcvs, ws, field_cot, None, False)


def newton(fields, s, dx, nn3, mn, sources, v, rcvs, ws=None, field_cot=None, row_weights=None):
    """J^T W J v + hvp(v): row_weights[e] one value per receiver of event e (or None: W = I, no product formed)"""
    return _product(fields, s, dx, nn3, mn, sources, v, rcvs, ws, field_cot, row_weights, True)
