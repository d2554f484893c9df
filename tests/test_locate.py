"""The grid-search hypocentre location without a device: what the cases of tests/test_locate_gpu.py decide, asserted on
oracle fields (eps = 1e-15) with the restatement of tests/locate_reference.py, so that the device test cannot pass by luck of geometry;
the box numbering, sw == 0 and the mirror tie of the definition; every argument error of the Python layer and of the C entries that can be
told before a device is needed; the new symbols; and inversion.locate on a stand-in tape built from oracle fields."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import locate_cases as LC  # noqa: E402
import locate_reference as LR  # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
NEW = ("ttcr_fsm_loc_geometry", "ttcr_fsm_loc_shape", "ttcr_fsm_loc_grid", "ttcr_fsm_loc_release")
# inversion.locate on the stand-in, noise-free picks at off-node points of the smooth model, refine = 10: the worst distance of a final
# point from the truth measured on these cases was 6.97e-6 (fp32 fields) and 1.92e-7 (fp64) in units of dx -- where the fields' own
# rounding leaves the minimum --; the bound is twice that
FINAL_ERROR_DX = {np.dtype(np.float32): 2 * 6.97e-6, np.dtype(np.float64): 2 * 1.92e-7}

_FIELDS = {}


def fields(dt, kind="gradient", stations=None, origin=LC.ZERO):
    key = (np.dtype(dt), kind, stations is None, tuple(origin))
    if key not in _FIELDS:
        _FIELDS[key] = LC.oracle_fields(dt, LC.NN, LC.model(LC.NN, kind), LC.STATIONS if stations is None else stations, origin=origin)
    return _FIELDS[key]


@DTYPES
def test_the_base_case_decides(dt):
    T = fields(dt)
    node, t0, mis, vol = LR.grid_search(T, LC.NN, LR.csr_of(*LC.base_picks(T)))
    assert LC.TRUE_NODES == (LC.node_of(LC.NN, 4, 3, 6), 0, 719, LC.node_of(LC.NN, 8, 0, 9))
    assert list(node) == list(LC.TRUE_NODES) * 2 + [0]
    assert np.all(mis == 0) and not np.any(np.signbit(mis))
    assert np.all(t0[:4] == 0) and np.all(t0[4:8] == LC.T_ORIGIN)
    for q in range(8):   # phi == +0 at exactly one node, the runner-up well away from it
        v = np.sort(vol[q].ravel())
        assert (vol[q] == 0).sum() == 1 and 8e-4 < v[1] < 1e-2, (q, v[:3])
    assert np.all(vol[8] == 0) and vol[8].size == 720           # one pick: phi == +0 at every node, the lowest node wins


@DTYPES
def test_mirror_tie_of_the_oracle_fields(dt):
    T = fields(dt, "homogeneous", LC.MIRROR_STATIONS)
    i, j, k = LC.MIRROR_TRUE
    true, mirror = LC.node_of(LC.NN, i, j, k), LC.node_of(LC.NN, i, j, 2 * LC.MIRROR_PLANE - k)
    # the oracle's fields of stations on nodes of the plane k = 5 are mirror-symmetric about it to the bit
    T3 = T.reshape(-1, LC.NN[2], LC.NN[1], LC.NN[0])
    for d in range(1, 5):
        assert LC.same_bits(T3[:, LC.MIRROR_PLANE - d], T3[:, LC.MIRROR_PLANE + d])
    node, t0, mis, vol = LR.grid_search(T, LC.NN, LR.csr_of(*LC.picks_at(T, true)))
    assert mirror < true and list(node) == [mirror] and mis[0] == 0
    assert sorted(np.flatnonzero(vol[0].ravel() == 0)) == [mirror, true]
    # with the lower one outside the box the true node is returned
    assert list(LR.grid_search(T, LC.NN, LR.csr_of(*LC.picks_at(T, true)), ((0, 9), (0, 8), (4, 10)))[0]) == [true]


def test_box_numbering_and_sw_zero():
    T = fields(np.float32)
    rng = np.random.default_rng(3)
    p = LC.join(LC.picks_at(T, 100, hypo=0), LC.picks_at(T, 650, fields=[4, 1, 1, 3], weights=[1, 0, 2, 0.5], hypo=1),
                LC.picks_at(T, 5, weights=np.zeros(5), hypo=3))
    p = (p[0], p[1], p[2] + 0.01 * rng.standard_normal(p[2].size), p[3])
    whole = LR.grid_search(T, LC.NN, LR.csr_of(*p, n_hypo=5))
    assert list(whole[0][2:]) == [-1, -1, -1] and np.all(whole[1][2:] == 0) and np.all(whole[2][2:] == 0) and np.all(whole[3][2:] == 0)
    assert not np.any(np.signbit(whole[3][2:])) and whole[3].shape == (5, 10, 8, 9)
    box = ((2, 7), (1, 6), (3, 9))
    nodes = LR.box_nodes(LC.NN, box)
    assert nodes[0] == LC.node_of(LC.NN, 2, 1, 3) and nodes[1] == nodes[0] + 1 and nodes[5] == LC.node_of(LC.NN, 2, 2, 3)
    assert nodes[25] == LC.node_of(LC.NN, 2, 1, 4) and nodes.size == 150 and np.all(np.diff(nodes) > 0)
    part = LR.grid_search(T, LC.NN, LR.csr_of(*p, n_hypo=5), box)
    assert part[3].shape == (5, 6, 5, 5) and LC.same_bits(part[3], whole[3][:, 3:9, 1:6, 2:7])
    for q in range(2):   # the node of the whole grid is reported, and it is the first of the smallest of the box
        flat = whole[3][q].ravel()[nodes]
        assert part[0][q] == nodes[np.argmin(flat)] and part[2][q] == flat.min()
    # the grouping is stable: the picks of a hypocentre stay in ascending pick index, and the order of the sums shows in the bits
    off, fld, tm, wt = LR.csr_of(*p, n_hypo=5)
    assert list(off) == [0, 5, 9, 9, 14, 14] and list(fld[5:9]) == [4, 1, 1, 3] and list(wt[5:9]) == [1, 0, 2, 0.5]


def test_python_layer_refuses_bad_arguments_before_any_device_call():
    from ttcr_amd.rgrid import FieldTape

    ok = dict(pick_hypo=[0, 0, 1], pick_field=[0, 1, 4], pick_time=[1.0, 2.0, 3.0], pick_weight=[1.0, 0.0, 2.0], n_hypo=None, box=None)
    nq, off, fld, tm, wt, b6 = FieldTape.locate_csr(5, LC.NN, **ok)
    assert nq == 2 and list(off) == [0, 2, 3] and b6 == [0, 9, 0, 8, 0, 10] and off.dtype == np.int64 and tm.dtype == np.float64
    bad = [("pick_field", dict(pick_field=[0, 1, 5])), ("pick_field", dict(pick_field=[0, -1, 4])), ("pick_field", dict(pick_field=[0.0, 1.0, 2.0])),
           ("pick_time", dict(pick_time=[1.0, np.nan, 3.0])), ("pick_time", dict(pick_time=[1.0, np.inf, 3.0])),
           ("pick_weight", dict(pick_weight=[1.0, -1e-300, 2.0])), ("pick_weight", dict(pick_weight=[1.0, np.inf, 2.0])),
           ("pick_weight", dict(pick_weight=[1.0, np.nan, 2.0])), ("pick_hypo", dict(pick_hypo=[0, -1, 1])),
           ("pick_hypo", dict(pick_hypo=[[0, 0, 1]])), ("one value per pick", dict(pick_time=[1.0, 2.0])),
           ("one value per pick", dict(pick_weight=[1.0])), ("n_hypo", dict(n_hypo=1)), ("n_hypo", dict(n_hypo=2.5)),
           ("n_hypo", dict(n_hypo=2 ** 22 + 1)), ("box", dict(box=((0, 10), (0, 8), (0, 10)))), ("box", dict(box=((-1, 9), (0, 8), (0, 10)))),
           ("box", dict(box=((0, 9), (3, 3), (0, 10)))), ("box", dict(box=((0, 9), (0, 8), (6, 2)))), ("box", dict(box=((0, 9), (0, 8)))),
           ("box", dict(box=(0, 9, 0, 8, 0, 10)))]
    for word, change in bad:
        with pytest.raises(ValueError, match=word):
            FieldTape.locate_csr(5, LC.NN, **dict(ok, **change))


def test_c_entries_refuse_bad_arguments_before_the_device():
    from ttcr_amd import build, _lib

    build.build()
    lib = _lib.load()
    node, t0, mis = (C.c_longlong * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    good = dict(off=[0, 2, 3], field=[0, 1, 0], time=[1.0, 2.0, 3.0], weight=[1.0, 0.0, 2.0], node=node, t0=t0, mis=mis)

    def call(**change):
        a = dict(good, **change)
        arr = lambda v, ct: None if v is None else (ct * len(v))(*v)   # noqa: E731
        st = lib.ttcr_fsm_loc_grid(None, 2, arr(a["off"], C.c_longlong), arr(a["field"], C.c_int), arr(a["time"], C.c_double),
                                   arr(a["weight"], C.c_double), None, a["node"], a["t0"], a["mis"], None, 0)
        return st, _lib.last_error()
    # everything that does not need the tape is told first, each naming its argument; then the tape
    for change, word in [(dict(off=None), "null hypo_off"), (dict(node=None), "null node_out"), (dict(t0=None), "null t0_out"),
                         (dict(mis=None), "null misfit_out"), (dict(off=[1, 2, 3]), "hypo_off"), (dict(off=[0, 3, 2]), "hypo_off"),
                         (dict(field=None), "null pick_field"), (dict(time=None), "null pick_time"), (dict(time=[1.0, float("nan"), 3.0]), "pick_time"),
                         (dict(time=[1.0, float("inf"), 3.0]), "pick_time"), (dict(weight=[1.0, -0.5, 2.0]), "pick_weight"),
                         (dict(weight=[1.0, float("nan"), 2.0]), "pick_weight"), (dict(weight=[float("inf"), 1.0, 2.0]), "pick_weight"),
                         (dict(), "null tape"), (dict(weight=None), "null tape")]:
        st, msg = call(**change)
        assert st == 1 and msg.startswith(word), (change, st, msg)
    nn, dx, o = (C.c_int * 3)(), C.c_double(0), (C.c_double * 3)()
    assert lib.ttcr_fsm_loc_geometry(None, nn, C.byref(dx), o) == 1 and _lib.last_error() == "null tape"
    a = C.c_int(0)
    assert lib.ttcr_fsm_loc_shape(None, C.byref(a), C.byref(a), C.byref(a)) == 1
    assert lib.ttcr_fsm_loc_release(None) == 1 and _lib.last_error() == "null tape"


def test_new_symbols_in_header_pxd_and_symbols():
    from ttcr_amd import _lib

    with open(os.path.join(ROOT, "include", "ttcr_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "integration", "ttcr_amd.pxd")) as f:
        pxd = f.read()
    for name in NEW:
        assert name in _lib.SYMBOLS and not name.startswith("ttcr_fsm_adjoint_")
        assert len(re.findall(r"^int %s\(" % name, header, re.M)) == 1 and len(re.findall(r"^    int %s\(" % name, pxd, re.M)) == 1
    from ttcr_amd.rgrid import FieldTape

    for name in ("geometry", "locate_grid", "node_coordinates", "release_locate", "locate_shape", "locate_csr"):
        assert hasattr(FieldTape, name)


# ---- inversion.locate on a stand-in tape
def _noise_free(stand_in, true, t_origin=3.0):
    nf = stand_in.n_events
    hyp, fld = np.repeat(np.arange(len(true)), nf), np.tile(np.arange(nf), len(true))
    tt = stand_in.receiver_eval(np.repeat(true, nf, axis=0), fld, return_grad=False).astype(np.float64)
    return hyp, fld, t_origin + tt, 1.0 + 0.5 * (fld % 3)


def _true_points(origin=LC.ZERO):
    rng = np.random.default_rng(37)
    return np.asarray(origin) + rng.uniform(0.6, np.array(LC.NN) - 1.6, (8, 3)) * LC.DX


@DTYPES
def test_locate_refine_zero_is_the_start_and_the_misfit_never_increases(dt):
    from ttcr_amd import inversion

    st = LR.StandInTape(list(fields(dt, "smooth")), LC.NN, LC.DX)
    true = _true_points()
    picks = _noise_free(st, true)
    t0, xyz, mis, info = inversion.locate(st, *picks, refine=0)
    assert LC.same_bits(xyz, info["start_xyz"]) and LC.same_bits(mis, info["start_misfit"]) and np.all(info["iterations"] == 0)
    # the start is the centre of a cell that touches the grid search's node: half a spacing from it on every axis
    assert np.all(np.abs(xyz - st.node_coordinates(info["node"])) == 0.5 * LC.DX)
    # ... the best of the up to 8: no other centre around the node has a smaller misfit
    hyp, fld, tm, wt = picks
    for q in range(len(true)):
        k = hyp == q
        for s in np.ndindex(2, 2, 2):
            c = st.node_coordinates(info["node"][q:q + 1])[0] + (np.array(s) - 0.5) * LC.DX
            if np.all(c > 0) and np.all(c < (np.array(LC.NN) - 1) * LC.DX):
                tt = st.receiver_eval(np.tile(c, (k.sum(), 1)), fld[k], return_grad=False).astype(np.float64)
                assert LR.misfit(tt[:, None], tm[k], wt[k])[2][0] >= mis[q]
    last = mis
    for refine in range(1, 12):
        st.evals = 0
        t0r, xyzr, misr, infor = inversion.locate(st, *picks, refine=refine)
        assert st.evals <= 1 + refine                               # one receiver_eval call for the start, one per iteration
        assert np.all(misr <= last) and np.all(infor["iterations"] <= refine) and LC.same_bits(infor["start_misfit"], mis)
        last = misr
    assert np.all(last < mis)


@DTYPES
def test_locate_ends_closer_to_the_truth_than_it_starts(dt):
    from ttcr_amd import inversion

    st = LR.StandInTape(list(fields(dt, "smooth")), LC.NN, LC.DX)
    true = _true_points()
    t0, xyz, mis, info = inversion.locate(st, *_noise_free(st, true), refine=10)
    start = np.linalg.norm(info["start_xyz"] - true, axis=1)
    final = np.linalg.norm(xyz - true, axis=1)
    print("locate on the stand-in (%s): worst start error %.3g dx, worst final error %.3g dx, worst |t0 - 3| %.3g"
          % (np.dtype(dt).name, start.max() / LC.DX, final.max() / LC.DX, np.abs(t0 - 3.0).max()))
    assert np.all(final < start)
    assert final.max() / LC.DX <= FINAL_ERROR_DX[np.dtype(dt)]


def test_locate_box_dead_hypocentres_and_argument_errors():
    from ttcr_amd import inversion

    st = LR.StandInTape(list(fields(np.float32, "smooth")), LC.NN, LC.DX)
    true = _true_points()[:3]
    hyp, fld, tm, wt = _noise_free(st, true)
    wt = np.where(hyp == 1, 0.0, wt)                                 # hypocentre 1: all weights zero; hypocentre 3: no picks
    box = ((0, 9), (0, 8), (2, 3))                                    # one node plane: the start may leave it, the node may not
    t0, xyz, mis, info = inversion.locate(st, hyp, fld, tm, wt, n_hypo=4, box=box, refine=3)
    assert list(info["node"][[1, 3]]) == [-1, -1] and np.all(np.isnan(xyz[[1, 3]])) and np.all(t0[[1, 3]] == 0) and np.all(mis[[1, 3]] == 0)
    assert np.all(info["node"][[0, 2]] // 72 == 2) and np.all(np.isfinite(xyz[[0, 2]]))
    for change, word in [(dict(refine=-1), "refine"), (dict(refine=1.5), "refine"), (dict(box=((0, 9), (0, 8), (3, 3))), "box"), (dict(n_hypo=2), "n_hypo")]:
        with pytest.raises(ValueError, match=word):
            inversion.locate(st, hyp, fld, tm, wt, **dict(dict(n_hypo=4, refine=3), **change))
    with pytest.raises(ValueError, match="pick_field"):
        inversion.locate(st, hyp, fld + 5, tm, wt)
