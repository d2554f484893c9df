"""Numpy restatement of the forward mode of the first-order 3-D node solver's linearisation (the device side is
ttcr_amd/csrc/fsm_adjoint.hip): mu = dT/ds . ds per event and dtt = the receiver rows of it.  Everything is computed in the dtype asked
for, every product, difference, quotient and sum rounded on its own, in the order of the definition; the nodes of an event are processed
in ascending T (stable argsort), so that every mu[u] a node gathers is final when it is read.

Conventions as in adjoint_reference.py, whose couplings, frozen_nodes and stencil are used here.
"""
import numpy as np

import adjoint_reference as AR


def tangent_event(T, s, dx, nn3, frozen, ds):
    """mu of one event: T the solved field, s the node slowness, frozen {node: d}, ds the perturbation; all flat, node order"""
    dt = T.dtype
    dx = dt.type(dx)
    nnx, nny, nnz = nn3
    upper, active, D, fz = AR.couplings(T, nn3, frozen)
    if np.any(~fz & ~(active[0] | active[1] | active[2])):
        raise RuntimeError('a node that is not frozen has no upwind neighbour: the field is not a solved one')
    stride = (1, nnx, nnx * nny)
    s = np.asarray(s, dtype=dt).ravel()
    ds = np.asarray(ds, dtype=dt).ravel()
    own = ((dx * (s * dx).astype(dt)).astype(dt) * ds).astype(dt)
    mu = np.zeros(T.size, dtype=dt)
    for m in np.argsort(T, kind='stable'):
        if fz[m]:
            mu[m] = dt.type(dt.type(frozen[m]) * ds[m])
            continue
        acc = own[m]
        tm = T[m]
        for axis in range(3):
            if active[axis][m]:
                u = m + stride[axis] if upper[axis][m] else m - stride[axis]
                acc = dt.type(acc + dt.type(mu[u] * dt.type(tm - T[u])))
        mu[m] = dt.type(acc / D[m])
    return mu


def rows(dtype, nn3, dx, mn, rcv, mu):
    """dtt of the receivers of one event: from +0, over the stencil entries in order, acc = fl(acc + fl(weight * mu[node]))"""
    dt = np.dtype(dtype)
    out = np.zeros(len(rcv), dtype=dt)
    for r, p in enumerate(np.asarray(rcv, dtype=dt).reshape(-1, 3)):
        nodes, wts = AR.stencil(dt, nn3, dx, mn, p)
        acc = dt.type(0)
        for m, wt in zip(nodes, wts):
            acc = dt.type(acc + dt.type(wt * mu[m]))
        out[r] = acc
    return out


def tangent(fields, s, dx, nn3, mn, sources, ds, rcvs=None):
    """(mus, dtts) for the events of a call: fields[e] the solved field of event e, sources[e] its points, rcvs[e] its receivers (or
    None: dtts is None); ds one value per node, shared by the events"""
    dt = np.dtype(fields[0].dtype)
    mus, dtts = [], []
    for e, T in enumerate(fields):
        fr = AR.frozen_nodes(dt, nn3, dx, mn, sources[e])
        mu = tangent_event(np.asarray(T, dtype=dt).ravel(), s, dx, nn3, fr, ds)
        mus.append(mu)
        if rcvs is not None:
            dtts.append(rows(dt, nn3, dx, mn, rcvs[e], mu))
    return mus, (dtts if rcvs is not None else None)
