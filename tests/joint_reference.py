"""Numpy restatement of the field tape's joint hypocentre-velocity system (the device side is joint_seed_kernel and the
JOINT relaxations of ttcr_amd/csrc/fsm_adjoint.hip and the joint solver of fsm_normal.hip): the joint tangent of a slowness perturbation
and a source perturbation from one pass over the nodes in ascending T, the joint Gauss-Newton product and conjugate gradients on the
regularised, column-scaled joint normal equations.  Everything is computed in the dtype asked for, every product, difference, quotient
and sum rounded on its own, in the order of the definition.  Built on the restatements it joins: tangent_reference (rows),
source_reference (frozen_sources, source_adjoint), adjoint_reference (couplings), cell_reference (A^T) and normal_reference (dot, smooth).

A joint vector is the model vector followed by (t0, x, y, z) of every source point in call order; the functions take and return its two
blocks as a pair (model vector, (n_points, 4) array).
"""
import math

import numpy as np

import adjoint_reference as AR
import cell_reference as CR
import normal_reference as NR
import source_reference as SR
import tangent_reference as TR


def joint_tangent_event(T, s, dx, nn3, fsrc, ds, dsrc):
    """mu of one event: a frozen node holds fl(fl(d ds) + sigma), sigma the frozen-node expression of SR.source_tangent_event; every
    other node the expression of TR.tangent_event.  fsrc = SR.frozen_sources(...); ds per node, dsrc (points of the event, 4)"""
    dt = T.dtype
    dx = dt.type(dx)
    nnx, nny, nnz = nn3
    upper, active, D, fz = AR.couplings(T, nn3, {m: v[0] for m, v in fsrc.items()})
    if np.any(~fz & ~(active[0] | active[1] | active[2])):
        raise RuntimeError('a node that is not frozen has no upwind neighbour: the field is not a solved one')
    stride = (1, nnx, nnx * nny)
    s = np.asarray(s, dtype=dt).ravel()
    ds = np.asarray(ds, dtype=dt).ravel()
    dsrc = np.asarray(dsrc, dtype=dt).reshape(-1, 4)
    own = ((dx * (s * dx).astype(dt)).astype(dt) * ds).astype(dt)
    mu = np.zeros(T.size, dtype=dt)
    for m in np.argsort(T, kind='stable'):
        if fz[m]:
            d, q, c = fsrc[m]
            sigma = dsrc[q, 0]
            for a in range(3):
                sigma = dt.type(sigma + dt.type(dt.type(s[m] * c[a]) * dsrc[q, 1 + a]))
            mu[m] = dt.type(dt.type(dt.type(d) * ds[m]) + sigma)
            continue
        acc = own[m]
        tm = T[m]
        for axis in range(3):
            if active[axis][m]:
                u = m + stride[axis] if upper[axis][m] else m - stride[axis]
                acc = dt.type(acc + dt.type(mu[u] * dt.type(tm - T[u])))
        mu[m] = dt.type(acc / D[m])
    return mu


def joint_tangent(fields, s, dx, nn3, mn, sources, ds, dsrc, rcvs=None):
    """(mus, dtts) for the events of a call, as TR.tangent and SR.source_tangent: ds one value per NODE (a cell tape hands over A ds),
    dsrc (n_points, 4) over the points of all events in call order"""
    dt = np.dtype(fields[0].dtype)
    dsrc = np.asarray(dsrc, dtype=dt).reshape(-1, 4)
    mus, dtts = [], []
    q0 = 0
    for e, T in enumerate(fields):
        n = len(np.asarray(sources[e]).reshape(-1, 3))
        fs = SR.frozen_sources(dt, nn3, dx, mn, sources[e])
        mu = joint_tangent_event(np.asarray(T, dtype=dt).ravel(), s, dx, nn3, fs, ds, dsrc[q0:q0 + n])
        q0 += n
        mus.append(mu)
        if rcvs is not None:
            dtts.append(TR.rows(dt, nn3, dx, mn, rcvs[e], mu))
    return mus, (dtts if rcvs is not None else None)


def scale_block(c, v, dtype):
    """fl(c * v) over a source block; c None: v itself, no multiplication"""
    dt = np.dtype(dtype)
    v = np.asarray(v, dtype=dt).reshape(-1, 4)
    if c is None:
        return v
    return (np.broadcast_to(np.asarray(c, dtype=dt), v.shape) * v).astype(dt)


def joint_product(fields, s, dx, nn3, mn, sources, rcvs, v_s, v_e, row_weights=None, source_scale=None, cells=None, to_nodes=None):
    """(g_s, g_e) of the joint Gauss-Newton product on a node tape, or on a cell tape with cells = (ncx, ncy, ncz) and to_nodes the
    averaging A (v_s then holds cells).  row_weights[e]: the weights of the rows of event e, or None."""
    dt = np.dtype(fields[0].dtype)
    ve = scale_block(source_scale, v_e, dt)
    ds = np.asarray(v_s, dtype=dt) if cells is None else np.asarray(to_nodes(v_s), dtype=dt)
    _, dtts = joint_tangent(fields, s, dx, nn3, mn, sources, ds, ve, rcvs=rcvs)
    ws = dtts if row_weights is None else [(np.asarray(rw, dtype=dt) * d).astype(dt) for rw, d in zip(row_weights, dtts)]
    g_s, g_e = SR.source_adjoint(fields, s, dx, nn3, mn, sources, rcvs=rcvs, ws=ws)
    if cells is not None:
        g_s = CR.nodes_to_cells(dt, cells, g_s)
    return g_s, scale_block(source_scale, g_e, dt)


def cg(product, rhs_s, rhs_e, dtype, smooth_op=None, smooth=0.0, damp=0.0, source_damp=None, source_scale=None, maxiter=20, rtol=1e-6):
    """Conjugate gradients from zero on the joint system.  product(p_s, p_e) returns (g_s, g_e) with the column scaling already inside
    (FieldTape.gauss_newton_joint(..., source_scale=source_scale), or joint_product); smooth_op(p_s) is R p_s.  source_damp and
    source_scale: None or arrays that broadcast to (n_points, 4).  Returns (x_s, x_e, info), info as FieldTape.solve_joint gives it
    without the pass counts."""
    dt = np.dtype(dtype)
    T = dt.type
    lam, mu = T(smooth), T(damp)
    rhs_s = np.asarray(rhs_s, dtype=dt).ravel()
    be = scale_block(source_scale, rhs_e, dt)
    npts = be.shape[0]
    nc = rhs_s.size
    delta = None
    if source_damp is not None and np.any(np.asarray(source_damp) != 0):
        delta = np.broadcast_to(np.asarray(source_damp, dtype=dt), (npts, 4)).ravel()

    def A(p):
        ps, pe = p[:nc], p[nc:]
        g_s, g_e = product(ps, pe.reshape(npts, 4))
        q_s = np.asarray(g_s, dtype=dt).ravel()
        if smooth != 0:
            q_s = q_s + lam * np.asarray(smooth_op(ps), dtype=dt)
        if damp != 0:
            q_s = q_s + mu * ps
        q_e = np.asarray(g_e, dtype=dt).ravel()
        if delta is not None:
            q_e = q_e + delta * pe
        q = np.concatenate([q_s, q_e])
        assert q.dtype == dt
        return q

    rhs = np.concatenate([rhs_s, be.ravel()])
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        x = np.zeros(rhs.size, dtype=dt)
        r = rhs.copy()
        p = r.copy()
        rho0 = NR.dot(rhs, rhs)
        rho = NR.dot(r, r)
        info = {'status': 1, 'iterations': 0, 'rho': [rho0, rho], 'pq': []}
        for _ in range(maxiter):
            if rho <= rtol * rtol * rho0:
                info['status'] = 0
                break
            q = A(p)
            pq = NR.dot(p, q)
            info['pq'].append(pq)
            if not (pq > 0) or not math.isfinite(pq):
                info['status'] = 2
                break
            aT = T(rho / pq)
            x = x + aT * p
            r = r - aT * q
            rho_new = NR.dot(r, r)
            bT = T(np.float64(rho_new) / np.float64(rho))
            p = r + bT * p
            rho = rho_new
            info['rho'].append(rho)
            info['iterations'] += 1
    assert x.dtype == dt
    return x[:nc], scale_block(source_scale, x[nc:], dt), info
