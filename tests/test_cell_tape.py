"""The field tape of cell grids without a device: the new entries of the C ABI are exported and declared and refuse NULL
arguments before any device call; the restated transpose of the cell-to-node averaging (tests/cell_reference.py, what the device is
compared with bit for bit) is the transpose of the oracle's cells_to_nodes3d, unit vector by unit vector and in the dot-product identity;
and the cell gradient A^T (node gradient of tests/adjoint_reference.py) is the derivative of what the oracle computes for a cell grid:
central finite differences agree with it to 1e-6 relative, the bound tests/test_adjoint.py uses for the node gradient."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as AR  # noqa: E402
import cell_reference as CR  # noqa: E402

CELL_SYMBOLS = ["ttcr_fsm_raytrace_multi_adjoint_cells", "ttcr_fsm_adjoint_model"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_cell_symbols_exported_and_declared(lib):
    from ttcr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttcr_amd.h")).read()
    pxd = open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")).read()
    for name in CELL_SYMBOLS:
        assert name + "(" in hdr, name
        assert name + "(" in pxd, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_null_arguments_are_value_errors_before_the_device(lib):
    from ttcr_amd import _lib

    n = C.c_size_t(0)
    d = C.c_int(0)
    fake = C.c_void_p(1234)   # never dereferenced: the argument checks come first
    assert lib.ttcr_fsm_raytrace_multi_adjoint_cells(None, 0, None, None, None, None, None, None, None) == _lib.ERR_VALUE
    assert "tape" in _lib.last_error()
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_raytrace_multi_adjoint_cells(None, 0, None, None, None, None, None, None, C.byref(h)) == _lib.ERR_VALUE
    assert h.value is None   # (*tape is cleared first)
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_raytrace_multi_adjoint_cells(fake, -1, None, None, None, None, None, None, C.byref(h)) == _lib.ERR_VALUE
    assert "adjoint_cells" in _lib.last_error() and h.value is None
    h = C.c_void_p(1234)
    assert lib.ttcr_fsm_raytrace_multi_adjoint_cells(fake, 1, None, None, None, None, None, None, C.byref(h)) == _lib.ERR_VALUE
    assert "null" in _lib.last_error() and h.value is None
    assert lib.ttcr_fsm_adjoint_model(None, C.byref(d), C.byref(n), C.byref(n)) == _lib.ERR_VALUE
    assert "null" in _lib.last_error()
    assert lib.ttcr_fsm_adjoint_model(fake, None, C.byref(n), C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_model(fake, C.byref(d), None, C.byref(n)) == _lib.ERR_VALUE
    assert lib.ttcr_fsm_adjoint_model(fake, C.byref(d), C.byref(n), None) == _lib.ERR_VALUE


def test_python_layer_takes_the_keyword():
    import inspect

    import ttcr_amd.autograd as ag
    from ttcr_amd.rgrid import _Grid3d

    for fn in (_Grid3d.raytrace_adjoint, ag.raytrace_adjoint, ag.raytrace_events):
        assert inspect.signature(fn).parameters["wrt"].default == "nodes", fn


# ---- A^T against the oracle's A
DOT_SHAPES = [(1, 1, 1), (1, 5, 3), (4, 1, 6), (5, 3, 1), (6, 8, 12), (5, 7, 4)]


def _n_nodes(nc):
    return (nc[0] + 1) * (nc[1] + 1) * (nc[2] + 1)


@pytest.mark.parametrize("nc", DOT_SHAPES, ids=lambda nc: "x".join(map(str, nc)))
def test_restated_transpose_against_the_oracle(nc):
    """|<A v, u> - <v, A^T u>| <= 1e-12 * sum of |terms| in fp64"""
    from oracle import oracle as O

    rng = np.random.default_rng(71 + nc[0] * 100 + nc[1] * 10 + nc[2])
    v = rng.standard_normal(nc[0] * nc[1] * nc[2])
    u = rng.standard_normal(_n_nodes(nc))
    Av = O.cells_to_nodes3d(np.float64, nc, v)
    Atu = CR.nodes_to_cells(np.float64, nc, u)
    assert Av.shape == u.shape and Atu.shape == v.shape
    lhs, rhs = Av @ u, v @ Atu
    scale = np.abs(Av) @ np.abs(u) + np.abs(v) @ np.abs(Atu)
    print("cells %s: <A v, u> - <v, A^T u> = %.2e, sum of |terms| %.2e" % ("x".join(map(str, nc)), abs(lhs - rhs), scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_restated_transpose_on_unit_vectors(dt):
    """for every node n of a 3 x 2 x 4-cell grid, A^T e_n is row n of the matrix whose columns are the oracle's A e_c: a wrong count on
    a corner, an edge or a face shows here"""
    from oracle import oracle as O

    nc = (3, 2, 4)
    n_cells, n_nodes = 24, _n_nodes(nc)
    A = np.zeros((n_nodes, n_cells), dtype=dt)
    for c in range(n_cells):
        e = np.zeros(n_cells, dtype=dt)
        e[c] = 1
        A[:, c] = O.cells_to_nodes3d(dt, nc, e)
    assert set(np.unique(A)) == {0.0, 0.125, 0.25, 0.5, 1.0}
    for n in range(n_nodes):
        e = np.zeros(n_nodes, dtype=dt)
        e[n] = 1
        col = CR.nodes_to_cells(dt, nc, e)
        assert col.dtype == np.dtype(dt) and np.array_equal(col, A[n]), (n, col, A[n])


# ---- the cell gradient against finite differences of the oracle (fp64, eps = 1e-15: the field is a fixed point of the sweeps)
DX = 0.5
MN = (0.0, 0.0, 0.0)
TOL = 1e-6    # the bound of tests/test_adjoint.py for the node gradient; the prototype of this check measured 1.6e-8 at worst
STEP = 1e-6
# cells per axis, source points in units of dx
FD_CASES = {
    "20x20x20": ((20, 20, 20), [[6.6, 8.2, 11.4]]),
    "12x9x14_two_points": ((12, 9, 14), [[3.3, 4.1, 5.7], [3.6, 4.2, 5.4]]),
    "7x1x5_thin": ((7, 1, 5), [[2.6, 0.4, 1.3]]),
    "1x1x1": ((1, 1, 1), [[0.3, 0.6, 0.2]]),
}


def _rough_cells(nc, rng):
    """a smooth trend times 1 +- 30 % noise, one value per cell, flat, x fastest"""
    ax = [0.5 * (np.arange(n) + 0.5) for n in nc]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    s = 0.5 + 0.02 * X + 0.015 * Y + 0.03 * Z + 0.05 * np.sin(0.9 * X) * np.cos(0.7 * Y + 0.3 * Z)
    return (s * (1.0 + 0.30 * rng.uniform(-1, 1, s.shape))).flatten("F")


def _solve(nc, sc, src, rcv):
    from oracle import oracle as O

    o = O.solve3d(np.float64, nc, DX, MN, sc, src, rcv=rcv, eps=1e-15, maxit=200, cell_slowness=True)
    # (stopped by eps, not by maxit: the last sweeps moved the field by rounding only -- 6e-15 summed over the 20^3-cell grid)
    assert o["niter"] < 200 and o["change"][-1] <= 1e-13, (o["niter"], o["change"][-3:])
    return o


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_cell_gradient_is_the_derivative_of_the_oracle(case):
    from oracle import oracle as O

    nc, src = FD_CASES[case]
    nn3 = tuple(n + 1 for n in nc)
    src = np.array(src) * DX
    rng = np.random.default_rng(5)
    sc = _rough_cells(nc, rng)
    hi = np.array(nc) * DX
    rcv = rng.uniform(0.1 * hi, 0.9 * hi, (30, 3))
    w = rng.standard_normal(30)
    gfield = rng.standard_normal(int(np.prod(nn3)))
    dsc = sc * rng.standard_normal(sc.size)
    o = _solve(nc, sc, src, rcv)
    s = O.cells_to_nodes3d(np.float64, nc, sc)   # the node slowness the solver worked on
    g_rcv = CR.nodes_to_cells(np.float64, nc, AR.adjoint([o["tt"]], s, DX, nn3, MN, [src], rcvs=[rcv], ws=[w]))
    g_fld = CR.nodes_to_cells(np.float64, nc, AR.adjoint([o["tt"]], s, DX, nn3, MN, [src], field_cot=[gfield]))
    op, om = _solve(nc, sc + STEP * dsc, src, rcv), _solve(nc, sc - STEP * dsc, src, rcv)
    fd_rcv = (w @ op["tt_rcv"] - w @ om["tt_rcv"]) / (2 * STEP)
    fd_fld = (gfield @ op["tt"] - gfield @ om["tt"]) / (2 * STEP)
    e_rcv = abs(g_rcv @ dsc - fd_rcv) / abs(fd_rcv)
    e_fld = abs(g_fld @ dsc - fd_fld) / abs(fd_fld)
    print("cell gradient vs oracle finite differences, %s: receivers %.2e, field %.2e (bound %.0e)" % (case, e_rcv, e_fld, TOL))
    assert e_rcv <= TOL and e_fld <= TOL, (e_rcv, e_fld)
