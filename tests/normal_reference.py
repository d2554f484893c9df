"""Numpy restatement of the field tape's normal equations (the device side is ttcr_amd/csrc/fsm_normal.hip): the
smoothing operator R v = sum_d a_d K_d^T (K_d v) on a model vector in the tape's order (x fastest), the solver's inner product with its
fixed summation order, and the conjugate-gradient recurrence.  Vectors are in the dtype asked for, every product, difference, quotient
and sum rounded on its own, in the order of the definition; scalars of the recurrence are Python floats (fp64).  The product H p of the
recurrence is a callable: a dense matrix on the CPU, the device's own gauss_newton on the GPU.
"""
import math

import numpy as np

CHUNK = 1024     # elements of a chunk partial
THREADS = 256    # threads of a workgroup


def _axis(a, axis, ih2, m2ih2):
    """K^T (K a) along one axis of a 3-D array: rows ascending, the sum from its first term"""
    T = a.dtype.type
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    if n < 3:
        raise ValueError('second-order smoothing needs at least 3 parameters along every axis')
    c = np.clip(np.arange(n), 1, n - 2)
    y = ((a[c - 1] + a[c + 1]) - T(2) * a[c]) * ih2
    z = np.empty_like(a)
    for i in range(n):
        terms = []
        if i <= 2:
            terms.append((m2ih2 if i == 1 else ih2) * y[0])
        for r in (i - 1, i, i + 1):
            if 1 <= r <= n - 2:
                terms.append((m2ih2 if r == i else ih2) * y[r])
        if i >= n - 3:
            terms.append((m2ih2 if i == n - 2 else ih2) * y[n - 1])
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        z[i] = acc
    return np.moveaxis(z, 0, axis)


def smooth(v, shape, dx, weights=(1., 1., 1.), dtype=None):
    """R v: v flat, x fastest, shape = (mx, my, mz) parameters along x, y, z; the result flat in the same order"""
    dt = np.dtype(dtype if dtype is not None else np.asarray(v).dtype)
    T = dt.type
    mx, my, mz = shape
    a = np.asarray(v, dtype=dt).reshape(mz, my, mx)
    ih2 = T(1.0 / (float(dx) * float(dx)))
    m2ih2 = T(-2) * ih2
    with np.errstate(over='ignore', invalid='ignore'):
        zx, zy, zz = (_axis(a, ax, ih2, m2ih2) for ax in (2, 1, 0))
        ax_, ay_, az_ = (T(w) for w in weights)
        out = (ax_ * zx + ay_ * zy) + az_ * zz
    assert out.dtype == dt
    return out.ravel()


def _halve(s):
    """s (rows, 256) -> (rows,): s[t] += s[t + stride] for stride = 128 .. 1"""
    s = s.copy()
    stride = THREADS // 2
    while stride >= 1:
        s[:, :stride] += s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0]


def dot(a, b):
    """<a, b> as the device sums it: a Python float"""
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64) and a.size == b.size
    n = a.size
    n_chunks = max(1, -(-n // CHUNK))
    e = np.zeros(n_chunks * CHUNK, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        e[:n] = a.astype(np.float64) * b.astype(np.float64)
        e = e.reshape(n_chunks, 4, THREADS)
        partial = _halve(((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3])
        rounds = -(-n_chunks // THREADS)
        p = np.zeros(rounds * THREADS, dtype=np.float64)
        p[:n_chunks] = partial
        acc = np.zeros((1, THREADS), dtype=np.float64)
        for row in p.reshape(rounds, THREADS):
            acc[0] += row
        return float(_halve(acc)[0])


def cg(hprod, rhs, dtype, smooth_op=None, smooth=0.0, damp=0.0, x0=None, maxiter=20, rtol=1e-6):
    """Conjugate gradients on (H + smooth R + damp I) x = rhs: hprod(p) is H p, smooth_op(p) is R p (needed for smooth != 0).  Returns
    (x, info) with info as FieldTape.solve_normal(return_info=True) gives it, without the pass counts."""
    dt = np.dtype(dtype)
    T = dt.type
    lam, mu = T(smooth), T(damp)

    def A(p):
        q = np.asarray(hprod(p), dtype=dt).ravel()
        if smooth != 0:
            q = q + lam * np.asarray(smooth_op(p), dtype=dt)
        if damp != 0:
            q = q + mu * p
        assert q.dtype == dt
        return q

    rhs = np.asarray(rhs, dtype=dt).ravel()
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        if x0 is None:
            x = np.zeros(rhs.size, dtype=dt)
            r = rhs.copy()
        else:
            x = np.array(x0, dtype=dt).ravel()
            r = rhs - A(x)
        p = r.copy()
        rho0 = dot(rhs, rhs)
        rho = dot(r, r)
        info = {'status': 1, 'iterations': 0, 'rho': [rho0, rho], 'pq': []}
        for _ in range(maxiter):
            if rho <= rtol * rtol * rho0:
                info['status'] = 0
                break
            q = A(p)
            pq = dot(p, q)
            info['pq'].append(pq)
            if not (pq > 0) or not math.isfinite(pq):
                info['status'] = 2
                break
            aT = T(rho / pq)
            x = x + aT * p
            r = r - aT * q
            rho_new = dot(r, r)
            bT = T(np.float64(rho_new) / np.float64(rho))
            p = r + bT * p
            rho = rho_new
            info['rho'].append(rho)
            info['iterations'] += 1
    assert x.dtype == dt
    return x, info
