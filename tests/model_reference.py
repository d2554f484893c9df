"""Numpy restatement of the field tape's coarse model grid (the device side is ttcr_amd/csrc/fsm_model.hip): the trilinear
prolongation P from m = (mx, my, mz) model nodes onto n = (nx, ny, nz) fine nodes (both flat, x fastest), its transpose in three stages,
and the smoothing operator of a model tape.  Every product and sum is rounded in the dtype asked for, in the order of the definition; a
term whose weight is exactly 0 is left out of every sum.
"""
import numpy as np

import normal_reference as NR


def axis_stencil(n, m, dtype):
    """(I, wl, wh) of every fine index of one axis: 64-bit integer arithmetic, each quotient in double and rounded to dtype once"""
    T = np.dtype(dtype).type
    if not 1 <= m <= n:
        raise ValueError('1 <= m <= n')
    if m == 1:
        return np.zeros(n, dtype=np.int64), np.ones(n, dtype=dtype), np.zeros(n, dtype=dtype)
    i = np.arange(n, dtype=np.int64)
    q = i * np.int64(m - 1)
    I, r = q // np.int64(n - 1), q % np.int64(n - 1)
    last = I == m - 1
    I = np.where(last, m - 2, I)
    r = np.where(last, n - 1, r)
    wl = (np.float64(n - 1) - r.astype(np.float64)) / np.float64(n - 1)
    wh = r.astype(np.float64) / np.float64(n - 1)
    return I, wl.astype(T), wh.astype(T)


def _lerp(wl, wh, a, b):
    """the sum, lower index first, of the non-zero-weight terms fl(wl a), fl(wh b); wl, wh broadcast against a, b"""
    with np.errstate(over='ignore', invalid='ignore'):
        lo, hi = wl * a, wh * b
        both = lo + hi
    return np.where(wh == 0, lo, np.where(wl == 0, hi, both))


def prolong(v, n, m, dtype):
    """s = P v: v flat (mx my mz values, x fastest) -> s flat (nx ny nz values)"""
    dt = np.dtype(dtype)
    a = np.asarray(v, dtype=dt).reshape(m[2], m[1], m[0])
    for axis, d in ((2, 0), (1, 1), (0, 2)):   # lerp_x, then lerp_y, then lerp_z
        I, wl, wh = axis_stencil(n[d], m[d], dt)
        hi = np.minimum(I + 1, m[d] - 1)        # (read only where wh != 0)
        sh = [1, 1, 1]
        sh[axis] = n[d]
        a = _lerp(wl.reshape(sh), wh.reshape(sh), np.take(a, I, axis=axis), np.take(a, hi, axis=axis)).astype(dt)
    return a.ravel()


def _stage(g, axis, n, m, dt):
    """one stage of P^T along `axis` of a 3-D array: per model index the serial sum over the fine k, ascending, from the first term"""
    I, wl, wh = axis_stencil(n, m, dt)
    g = np.moveaxis(g, axis, 0)
    out = np.zeros((m,) + g.shape[1:], dtype=dt)
    first = np.ones(m, dtype=bool)
    with np.errstate(over='ignore', invalid='ignore'):
        for k in range(n):
            for K, w in ((int(I[k]) + 1, wh[k]), (int(I[k]), wl[k])):   # (two different K: the order between them does not matter)
                if w == 0 or K >= m:
                    continue
                p = w * g[k]
                out[K] = p if first[K] else out[K] + p
                first[K] = False
    return np.moveaxis(out, 0, axis)


def restrict(g, n, m, dtype):
    """g_m = P^T g: g flat (nx ny nz values) -> flat mx my mz values; stage z, then y, then x"""
    dt = np.dtype(dtype)
    a = np.asarray(g, dtype=dt).reshape(n[2], n[1], n[0])
    for axis, d in ((0, 2), (1, 1), (2, 0)):
        a = _stage(a, axis, n[d], m[d], dt)
    return a.ravel()


def stage_lengths(n, m):
    """(L_x, L_y, L_z): the longest sum of each stage of P^T"""
    out = []
    for d in range(3):
        I, wl, wh = axis_stencil(n[d], m[d], np.float64)
        cnt = np.zeros(m[d], dtype=np.int64)
        for k in range(n[d]):
            if wl[k] != 0:
                cnt[I[k]] += 1
            if wh[k] != 0:
                cnt[I[k] + 1] += 1
        out.append(int(cnt.max()))
    return tuple(out)


def weight_matrix(n, m, dtype):
    """P as a dense fp64 matrix (fine nodes x model nodes) of the exact products w_x w_y w_z of the rounded per-axis weights"""
    ax = []
    for d in range(3):
        I, wl, wh = axis_stencil(n[d], m[d], dtype)
        A = np.zeros((n[d], m[d]))
        for k in range(n[d]):
            if wl[k] != 0:
                A[k, I[k]] += float(wl[k])
            if wh[k] != 0:
                A[k, I[k] + 1] += float(wh[k])
        ax.append(A)
    return np.kron(ax[2], np.kron(ax[1], ax[0]))


def spacings(n, m, dx):
    """h_d = dx (n_d - 1) / (m_d - 1) in double for the axes with m_d >= 3 (None for the others, which R leaves out)"""
    return tuple(float(dx) * float(n[d] - 1) / float(m[d] - 1) if m[d] >= 3 else None for d in range(3))


def smooth(v, n, m, dx, weights, dtype):
    """R v on a model tape: per-axis ih2 = T(1 / (h_d h_d)); an axis with m_d < 3 has to have weight 0 and is not evaluated; the sum
    runs left to right over the evaluated axes in x, y, z order"""
    dt = np.dtype(dtype)
    T = dt.type
    a = np.asarray(v, dtype=dt).reshape(m[2], m[1], m[0])
    acc = None
    with np.errstate(over='ignore', invalid='ignore'):
        for d, axis in ((0, 2), (1, 1), (2, 0)):
            h = spacings(n, m, dx)[d]
            if h is None:
                if weights[d] != 0:
                    raise ValueError('a model axis with fewer than 3 nodes takes smoothing weight 0')
                continue
            ih2 = T(1.0 / (h * h))
            term = T(weights[d]) * NR._axis(a, axis, ih2, T(-2) * ih2)
            acc = term if acc is None else acc + term
    if acc is None:
        acc = np.zeros_like(a)
    assert acc.dtype == dt
    return acc.ravel()
