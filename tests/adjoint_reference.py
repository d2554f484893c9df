"""Numpy restatement of the adjoint-state gradient of the first-order 3-D node solver (the device side is
ttcr_amd/csrc/fsm_adjoint.hip).  Everything is computed in the dtype asked for, every product, difference, quotient and sum rounded on
its own, in the order of the definition; the nodes of an event are processed in descending T (stable argsort), so that every lam[n] a
node gathers is final when it is read.

Conventions: node m = (k * nny + j) * nnx + i (x fastest); nn3 = (nnx, nny, nnz); mn = (xmin, ymin, zmin); one spacing dx.
"""
import numpy as np

SMALL = 1.e-4
SMALL2 = 1.e-4 * 1.e-4


def _first_match(dt, cmin, dx, nn, v):
    """first node whose coordinate is within 1e-4 of v (the on-node test of the source initialisation), or -1"""
    est = (float(v) - float(cmin)) / float(dx)
    c = int(np.floor(est))
    span = int(np.ceil(SMALL / abs(float(dx)))) + 2
    for i in range(max(0, c - span), min(nn - 1, c + span + 1) + 1):
        diff = dt.type(cmin + dt.type(i) * dx) - v
        if float(abs(diff)) < SMALL:
            return i
    return -1


def locate(dtype, nn3, dx, mn, p):
    """(on_node, i, j, k): the node a source point lies on, or the cell that holds it"""
    dt = np.dtype(dtype)
    dx = dt.type(dx)
    p = [dt.type(v) for v in p]
    mn = [dt.type(v) for v in mn]
    f = [_first_match(dt, mn[a], dx, nn3[a], p[a]) for a in range(3)]
    if min(f) >= 0:
        return True, f[0], f[1], f[2]
    c = []
    for a in range(3):
        cmax = dt.type(mn[a] + dt.type(nn3[a] - 1) * dx)
        v = p[a]
        if float(cmax - v) < SMALL2:
            v = dt.type(float(cmax) - .5 * float(dx))
        c.append(int(SMALL2 + float(dt.type(v - mn[a]) / dx)))
    return False, c[0], c[1], c[2]


def frozen_nodes(dtype, nn3, dx, mn, pts):
    """{node: d}: the nodes the source initialisation froze for the points `pts` (in order) and the distance to the point that wrote
    each one last.  Box around the point minus the node (i, j, k) itself, which is skipped in both branches; the on-node node: d = 0."""
    dt = np.dtype(dtype)
    dx = dt.type(dx)
    mn = [dt.type(v) for v in mn]
    nnx, nny, nnz = nn3
    out = {}
    for p in np.asarray(pts, dtype=dt).reshape(-1, 3):
        on, i, j, k = locate(dt, nn3, dx, mn, p)
        b0 = -1 if on else 0
        if on:
            out[(k * nny + j) * nnx + i] = dt.type(0)
        for kk in range(k + b0, k + 2):
            for jj in range(j + b0, j + 2):
                for ii in range(i + b0, i + 2):
                    if not (0 <= ii < nnx and 0 <= jj < nny and 0 <= kk < nnz) or (ii, jj, kk) == (i, j, k):
                        continue
                    x = dt.type(mn[0] + dt.type(ii) * dx)
                    y = dt.type(mn[1] + dt.type(jj) * dx)
                    z = dt.type(mn[2] + dt.type(kk) * dx)
                    d2 = dt.type(dt.type(dt.type(x - p[0]) * dt.type(x - p[0]) + dt.type(y - p[1]) * dt.type(y - p[1])) +
                                 dt.type(z - p[2]) * dt.type(z - p[2]))
                    out[(kk * nny + jj) * nnx + ii] = dt.type(np.sqrt(np.float64(d2)))
    return out


def stencil(dtype, nn3, dx, mn, p):
    """nodes and weights of the receiver interpolation at p, in the order the device helper (interp3d_stencil) lists them: x outer, y,
    z inner; an axis the point lies on gives one plane and no factor; indices clamped to the last node; weight = z factor, then * y
    factor, then * x factor"""
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
    nodes, wts = [], []
    for ii in range(1 if on[0] else 2):
        for jj in range(1 if on[1] else 2):
            for kk in range(1 if on[2] else 2):
                s = (ii, jj, kk)
                c = [min(lo[a] + s[a], nn3[a] - 1) for a in range(3)]
                w = None
                for a in (2, 1, 0):
                    if on[a]:
                        continue
                    f = w2[a] if s[a] else w1[a]
                    w = f if w is None else dt.type(w * f)
                nodes.append((c[2] * nn3[1] + c[1]) * nn3[0] + c[0])
                wts.append(dt.type(1) if w is None else w)
    return nodes, wts


def seeds(dtype, nn3, dx, mn, rcv, w, field_cot=None):
    """g of one event: the field cotangent (or +0), then, for the receiver rows in order, w[row] * weight added to every node of the
    row's stencil, one serial chain"""
    dt = np.dtype(dtype)
    n = nn3[0] * nn3[1] * nn3[2]
    g = np.zeros(n, dtype=dt) if field_cot is None else np.array(field_cot, dtype=dt).reshape(n).copy()
    if w is not None:
        for r, p in enumerate(np.asarray(rcv, dtype=dt).reshape(-1, 3)):
            nodes, wts = stencil(dt, nn3, dx, mn, p)
            for m, wt in zip(nodes, wts):
                g[m] = dt.type(g[m] + dt.type(dt.type(w[r]) * wt))
    return g


def couplings(T, nn3, frozen):
    """per axis (x, y, z): upper[axis][m] (the upwind neighbour is the upper one), active[axis][m]; D[m]; all zero / False for frozen m"""
    nnx, nny, nnz = nn3
    dt = T.dtype
    T3 = T.reshape(nnz, nny, nnx)
    fz = np.zeros(T.size, dtype=bool)
    fz[list(frozen)] = True
    fz3 = fz.reshape(T3.shape)
    upper, active = [], []
    D = np.zeros(T3.shape, dtype=dt)
    for axis in range(3):
        ax = 2 - axis   # array axis of the grid axis
        pad = [(0, 0)] * 3
        pad[ax] = (1, 1)
        P = np.pad(T3, pad, constant_values=np.inf)
        lo = np.take(P, range(0, T3.shape[ax]), axis=ax)
        hi = np.take(P, range(2, T3.shape[ax] + 2), axis=ax)
        up = hi < lo   # tie: the lower index
        a = np.where(up, hi, lo)
        act = (a < T3) & ~fz3
        with np.errstate(invalid='ignore'):
            d = (T3 - a).astype(dt)
        D = np.where(act, (D + np.where(act, d, 0)).astype(dt), D)
        upper.append(up.ravel())
        active.append(act.ravel())
    return upper, active, D.ravel(), fz


def adjoint_event(T, s, dx, nn3, frozen, g):
    """(lam, grad_e) of one event: T the solved field, s the node slowness, frozen {node: d}, g the seeds; all flat, node order"""
    dt = T.dtype
    dx = dt.type(dx)
    nnx, nny, nnz = nn3
    upper, active, D, fz = couplings(T, nn3, frozen)
    if np.any(~fz & ~(active[0] | active[1] | active[2])):
        raise RuntimeError('a node that is not frozen has no upwind neighbour: the field is not a solved one')
    stride = (1, nnx, nnx * nny)
    m_all = np.arange(T.size)
    pos = (m_all % nnx, (m_all // nnx) % nny, m_all // (nnx * nny))
    # feeds[2 * axis + side][j]: neighbour n of j on that side (side 0: lower index) has j as its active upwind neighbour
    feeds = []
    for axis in range(3):
        for side in (0, 1):
            f = np.zeros(T.size, dtype=bool)
            if side == 0:
                j = m_all[pos[axis] > 0]
                n = j - stride[axis]
                f[j] = active[axis][n] & upper[axis][n]
            else:
                j = m_all[pos[axis] < nn3[axis] - 1]
                n = j + stride[axis]
                f[j] = active[axis][n] & ~upper[axis][n]
            feeds.append(f)
    offs = (-stride[0], stride[0], -stride[1], stride[1], -stride[2], stride[2])
    lam = np.array(g, dtype=dt).copy()
    any_feed = feeds[0] | feeds[1] | feeds[2] | feeds[3] | feeds[4] | feeds[5]
    for j in np.argsort(-T, kind='stable'):
        if not any_feed[j]:
            continue
        acc = lam[j]
        tj = T[j]
        for q in range(6):
            if feeds[q][j]:
                n = j + offs[q]
                acc = dt.type(acc + dt.type(dt.type(lam[n] * dt.type(T[n] - tj)) / D[n]))
        lam[j] = acc
    c = (dx * (s * dx).astype(dt)).astype(dt)
    with np.errstate(divide='ignore', invalid='ignore'):
        grad = ((lam * c).astype(dt) / D).astype(dt)
    for m, d in frozen.items():
        grad[m] = dt.type(dt.type(d) * lam[m])
    return lam, grad


def adjoint(fields, s, dx, nn3, mn, sources, rcvs=None, ws=None, field_cot=None):
    """d loss / d node slowness for the events of a call: fields[e] the solved field of event e, sources[e] its points, rcvs[e] / ws[e]
    its receivers and their cotangents (or None), field_cot[e] its field cotangent (or None).  Events summed ascending from +0."""
    dt = np.dtype(fields[0].dtype)
    s = np.asarray(s, dtype=dt).ravel()
    grad = np.zeros(s.size, dtype=dt)
    for e, T in enumerate(fields):
        fr = frozen_nodes(dt, nn3, dx, mn, sources[e])
        g = seeds(dt, nn3, dx, mn, None if rcvs is None else rcvs[e], None if ws is None else ws[e],
                  None if field_cot is None else field_cot[e])
        grad = (grad + adjoint_event(np.asarray(T, dtype=dt).ravel(), s, dx, nn3, fr, g)[1]).astype(dt)
    return grad
