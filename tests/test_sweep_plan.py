"""The kernel choice of the sweep launches (ttcr_fsm_sweep_plan, ttcr_amd/csrc/fsm_sweep_plan.h and fsm_sweep_dispatch.h), on the CPU.

One plan per launch picks the instantiation of fsm_sweep_persistent / fsm_sweep_tile, prints the name ttcr_fsm_last_kernel reports and
gives the launch geometry; the dispatcher says whether the library holds that instantiation.  Checked here without a device:

  recipes    every recipe with which a GPU test brings the host to launch a kernel it names -- the Inst rows of test_few_workgroups_gpu
             and test_weno_2d_gpu, the KERNELS table of test_chunk_dirty_gpu, the rows and the limit of test_long_axis_gpu -- yields
             that name, at the test's own shapes and slot counts, under the recipe's environment and options, for the batch of the last
             round of a call (the launch whose name the GPU test reads), and the library holds the kernel
  the sweep  dimension x precision x WENO x slots x batch x mode x skip x lone_chunk x arith x TTCR_FSM_PAIR on a small grid and on
             512^3 nodes (where the pair, probe and skip thresholds are all crossed): every plan names a kernel the library holds, or is
             the one documented refusal (option arith without whole-iteration launches); the name is well formed and says what the
             plan's fields say
  literals   four plans read off the rules, written out
"""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import few_workgroups_cases as fw
import long_axis_cases as la
import weno_2d_cases as wc

F32, F64 = 0, 1
WG_CAP = 2048   # 8 workgroups per compute unit of a 256-CU device
ENV_KEYS = ("TTCR_FSM_WGS", "TTCR_FSM_PAIR", "TTCR_FSM_PRE_MIN", "TTCR_FSM_TIME_ORDER_BELOW", "TTCR_FSM_MODE", "TTCR_FSM_SKIP",
            "TTCR_FSM_LONE_CHUNK", "TTCR_FSM_ARITH", "TTCR_FSM_PAIR_UNITS", "TTCR_FSM_WENO_CH4_MIN", "TTCR_FSM_WENO_C16_BELOW",
            "TTCR_FSM_F64_C16_BELOW", "TTCR_FSM_XS_LDS", "TTCR_FSM_XS_LDS_BELOW", "TTCR_FSM_SKIP_UNITS", "TTCR_FSM_SKIP_PROBE_UNITS",
            "TTCR_FSM_SKIP_ALL_DIRTY", "TTCR_FSM_NO_SW", "TTCR_FSM_LAYOUT_LO", "TTCR_FSM_LAYOUT_HI")
FIELDS = ("status", "wgs", "block", "dyn_lds", "tickets", "launches", "chunk", "skip", "xs", "pre", "ns", "ar")
PER_SWEEP, XS_BY_SWEEP, XS_BY_TIME = 0, 1, 2
PERSISTENT = re.compile(r"^fsm_sweep_persistent<(float|double),(\d+),(\d+),(\d+),(true|false),(true|false),([12]),([12]),(true|false),(true|false)(,1)?>$")
TILE = re.compile(r"^fsm_sweep_tile<(float|double),(\d+),(\d+),(\d+),(true|false)>$")


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


@pytest.fixture()
def env(monkeypatch):
    """the TTCR_FSM_* variables the plan reads: all unset, then as asked for"""
    def set_(**kw):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
    set_()
    return set_


def plan(lib, nodes, dtype, n_slots, batch, weno=0, stage=0, opts=None, layout=-1, wg_cap=WG_CAP, status_only=False):
    """the plan of a launch of `batch` entries on a grid of `nodes` ((nx, ny, nz) or (nx, nz)): dict of FIELDS + name"""
    from ttcr_amd import _lib

    dim = len(nodes)
    nnx, nny, nnz = nodes if dim == 3 else (nodes[0], 0, nodes[1])
    opts = opts or {}
    keys = (C.c_char_p * len(opts))(*[k.encode() for k in opts])
    vals = (C.c_double * len(opts))(*[float(v) for v in opts.values()])
    name = C.create_string_buffer(160)
    out = (C.c_longlong * len(FIELDS))()
    st = lib.ttcr_fsm_sweep_plan(dim, F64 if np.dtype(dtype) == np.float64 else F32, int(weno), nnx, nny, nnz, n_slots, keys, vals, len(opts), wg_cap,
                                 stage, batch, layout, name, len(name), out)
    if status_only:
        return st
    assert st == _lib.OK, _lib.last_error()
    return dict(zip(FIELDS, out), name=name.value.decode())


def last_batch(n_src, n_threads, ns):
    """batch entries of the last round of a call with n_src sources: the slot groups that hold a source of that round"""
    _, rounds = fw.held(list(range(n_src)), n_threads)
    return -(-len(rounds[-1]) // ns)


def check_recipe(lib, env, nodes, dtype, n_threads, n_src, weno, environment, opts, name):
    env(**environment)
    probe = plan(lib, nodes, dtype, n_threads, 1, weno=weno, stage=int(weno), opts=opts)   # (for the layout the grid takes)
    p = plan(lib, nodes, dtype, n_threads, last_batch(n_src, n_threads, probe["ns"]), weno=weno, stage=int(weno), opts=opts)
    assert p["name"] == name and p["status"] == 0, (p, name)
    return p


# ---------------------------------------------------------------------------------------------------------------- the recipes
def _few_workgroups():
    from test_few_workgroups_gpu import INSTANTIATIONS
    return INSTANTIATIONS


def _weno_2d():
    from test_weno_2d_gpu import INSTANTIATIONS
    return INSTANTIATIONS


@pytest.mark.parametrize("shape", fw.SHAPES, ids=["x".join(map(str, s)) for s in fw.SHAPES])
def test_recipes_of_test_few_workgroups_gpu(lib, env, shape):
    insts = _few_workgroups()
    assert len(insts) == 28
    for inst in insts:
        for wgs in (None, 1, 3, 0):
            p = check_recipe(lib, env, shape, inst.dtype, inst.n_threads, fw.N_SRC, 0, dict(inst.env, **({} if wgs is None else {"TTCR_FSM_WGS": wgs})),
                             inst.opts, inst.name)
            assert (p["ns"], p["chunk"], bool(p["xs"]), p["skip"], p["pre"]) == (inst.ns, inst.ch, inst.xs, inst.skip, inst.pre), (inst.id, p)
            units = p["wgs"] if wgs else None
            assert units is None or units <= wgs, (inst.id, wgs, p)   # (first-order 3-D kernels: TTCR_FSM_WGS caps the workgroups)
        p = check_recipe(lib, env, shape, inst.dtype, inst.n_threads, fw.N_SRC, 0, dict(inst.env, TTCR_FSM_TIME_ORDER_BELOW=0), inst.opts, inst.name)
        assert p["tickets"] == (XS_BY_SWEEP if inst.xs else PER_SWEEP), (inst.id, p)


def test_recipes_of_test_weno_2d_gpu(lib, env):
    insts = _weno_2d()
    assert len(insts) == 76
    for inst in insts:
        cases = [wc.MAIN_3D] + wc.OTHER_3D + [wc.CELLS_3D] if inst.dim == 3 else [wc.MAIN_2D, wc.XZ_2D] + wc.OTHER_2D + [wc.CELLS_2D]
        for c in cases:
            nodes = c["n"]   # (nodes, on cell grids as well)
            for extra in ({}, {"TTCR_FSM_TIME_ORDER_BELOW": 0}):
                p = check_recipe(lib, env, nodes, inst.dtype, inst.n_threads, wc.N_SRC, inst.weno, dict(inst.env, **extra), inst.opts, inst.name)
                assert (p["ns"], p["chunk"], bool(p["xs"]), p["skip"], p["pre"]) == (inst.ns, inst.ch, inst.xs, inst.skip, inst.pre), (inst.id, p)
                assert p["tickets"] == (PER_SWEEP if not inst.xs else XS_BY_SWEEP if extra else XS_BY_TIME), (inst.id, p)


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=["fp32", "fp64"])
def test_weno_stage_of_a_mode_0_grid(lib, env, dtype):
    """test_weno_2d_gpu.test_weno_grid_under_mode_0_takes_the_launch_per_sweep_kernel: the first-order stage is the tile kernel"""
    from test_weno_2d_gpu import Inst

    inst = Inst(dtype, 3, 2, 1, 8, False, 1, 0)
    check_recipe(lib, env, wc.MAIN_3D["n"], dtype, inst.n_threads, wc.N_SRC, 1, inst.env, {"mode": 0}, inst.name)
    env()
    p = plan(lib, wc.MAIN_3D["n"], dtype, inst.n_threads, inst.n_threads, weno=1, stage=0, opts={"mode": 0})
    assert TILE.match(p["name"]) and p["status"] == 0 and p["launches"] > 8, p


def test_recipes_of_test_chunk_dirty_gpu_and_test_long_axis_gpu(lib, env):
    from test_chunk_dirty_gpu import KERNELS, N_SRC, SHAPES

    assert len(KERNELS) == 5
    for kern, (dtype, slots, environment, opts, name) in KERNELS.items():
        rows = [(s, N_SRC) for s in SHAPES] + [(la.LONG["n"], la.n_src(la.LONG))]
        if kern in ("pairs-skip-pre", "fp64-pairs"):
            rows.append((la.LONGER["n"], la.n_src(la.LONGER)))
        for nodes, n_src in rows:
            for wgs in (None, 3):
                check_recipe(lib, env, nodes, dtype, slots, n_src, 0, dict(environment, **({} if wgs is None else {"TTCR_FSM_WGS": wgs})), opts, name)
            if kern == "arith1-pairs":   # (the control of that test: the same arithmetic, every chunk evaluated)
                check_recipe(lib, env, nodes, dtype, slots, n_src, 0, environment, dict(opts, skip=0), name.replace("true,true,1,2", "true,false,1,2"))
    for inst in _weno_2d():
        if inst.skip:
            for c in ([la.LONG_WENO] if inst.dim == 3 else la.LONG_2D):
                check_recipe(lib, env, c["n"], inst.dtype, inst.n_threads, la.n_src(c), inst.weno, inst.env, inst.opts, inst.name)


@pytest.mark.parametrize("pair", [None, "1"], ids=["one-field", "pairs"])
@pytest.mark.parametrize("dtype", la.DTYPES, ids=["fp32", "fp64"])
def test_the_limit_of_test_long_axis_gpu(lib, env, dtype, pair):
    """1024 F bricks skip, 1025 do not: two slots, option skip = 1, a batch of two and a lone source"""
    for c, skip in ((la.LIMIT[0], 1), (la.LIMIT[1], 0)):
        env(**({} if pair is None else {"TTCR_FSM_PAIR": pair}))
        for batch in ((1, 2) if pair is None else (1,)):
            p = plan(lib, c["n"], dtype, 2, batch, opts={"skip": 1})
            assert p["status"] == 0 and PERSISTENT.match(p["name"]), p
            assert (p["skip"], p["chunk"], p["ns"], bool(p["xs"])) == ((skip, 16, 1, True) if pair is None else (skip, 8, 2, True)), (c["name"], p)


# ------------------------------------------------------------------------------------------------------------------ the sweep
SLOTS = (1, 2, 3, 4, 5, 8, 9, 16, 64)
GRIDS = {3: [(37, 35, 41), (512, 512, 512)], 2: [(37, 41), (512, 512)]}


def _check_name(p, dtype, dim, stage):
    t = "double" if np.dtype(dtype) == np.float64 else "float"
    tf = {"true": True, "false": False}
    m = PERSISTENT.match(p["name"])
    if m is None:
        m = TILE.match(p["name"])
        assert m, p
        assert (m.group(1), tf[m.group(5)]) == (t, dim == 3) and stage == 0 and int(m.group(2)) * int(m.group(3)) == p["block"], p
        return False
    pj, pk = wc.TILE[(dim, np.dtype(dtype).name)]
    assert (m.group(1), int(m.group(2)), int(m.group(3)), tf[m.group(5)], int(m.group(7))) == (t, pj, pk, dim == 3, stage + 1), p
    assert (int(m.group(4)), tf[m.group(6)], int(m.group(8)), tf[m.group(9)], tf[m.group(10)], m.group(11) is not None) == \
        (p["chunk"], p["skip"] != 0, p["ns"], bool(p["xs"]), bool(p["pre"]), bool(p["ar"])), p
    assert p["block"] == pj * pk and p["wgs"] >= 1 and p["launches"] == (1 if p["xs"] else 8 if dim == 3 else 4), p
    assert p["tickets"] == (XS_BY_TIME if p["xs"] else PER_SWEEP) and (p["dyn_lds"] == 0 or p["xs"]), p
    return True


@pytest.mark.parametrize("pair", [None, "0", "1"], ids=["pair-unset", "pair-0", "pair-1"])
@pytest.mark.parametrize("weno", [0, 1], ids=["first-order", "weno"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("dim", [3, 2])
def test_every_plan_has_a_kernel_or_is_the_documented_refusal(lib, env, dim, dtype, weno, pair):
    if pair is not None:
        env(TTCR_FSM_PAIR=pair)
    plans = kernels = refused = 0
    for nodes, n_slots in itertools.product(GRIDS[dim], SLOTS):
        for mode, skip, lone, arith in itertools.product((0, 1, 2), (-1, 0, 1), (8, 16), (0, 1, 2)):
            opts = {"mode": mode, "skip": skip, "lone_chunk": lone, "arith": arith}
            fast = np.dtype(dtype) == np.float32 and (arith == 2 or (arith == 1 and not weno))
            for stage in range(1 + weno):
                first = plan(lib, nodes, dtype, n_slots, 1, weno=weno, stage=stage, opts=opts)
                pj, pk = wc.TILE[(dim, np.dtype(dtype).name)]
                units = n_slots * -(-nodes[1] // pj) * -(-nodes[-1] // pk)   # (the window of pair_units_min: fp32 8 and 9 slots, fp64 4 and 5)
                layouts = (-1, 0, 1) if dim == 3 and not weno and pair is None and 6144 < units <= 15360 else (-1,)
                for layout in layouts:
                    ns = {0: 1, 1: 2}.get(layout, first["ns"])
                    tile = mode == 0 and stage == 0
                    for batch in range(1, (n_slots if tile else -(-n_slots // ns)) + 1):
                        p = plan(lib, nodes, dtype, n_slots, batch, weno=weno, stage=stage, opts=opts, layout=layout)
                        what = (nodes, n_slots, opts, stage, layout, batch, p)
                        plans += 1
                        assert p["ns"] == ns, what
                        assert p["status"] == (1 if fast and mode != 2 else 0), what   # (never 2: no plan without a kernel)
                        refused += p["status"]
                        assert _check_name(p, dtype, dim, stage) == (not tile), what
                        assert bool(p["ar"]) == (fast and mode == 2 and (ns == 1 or (stage == 0 and dim == 3))), what
                        kernels += 1
                    if not tile:   # (one entry more than the grid has slot groups)
                        assert plan(lib, nodes, dtype, n_slots, -(-n_slots // ns) + 1, weno=weno, stage=stage, opts=opts, layout=layout, status_only=True) != 0
    assert plans == kernels and plans > 5000 and (refused > 0) == (np.dtype(dtype) == np.float32), (plans, refused)


def test_thresholds_crossed_on_512_cubed(lib, env):
    """pairs from 7 slots on (slots x 1 024 patches > 6 144) with the window up to 15; the probe window of a lone source; skipping by
    default from two entries on; the layouts of a grid in the window"""
    n = (512, 512, 512)
    env()
    assert [plan(lib, n, np.float32, s, 1)["ns"] for s in (1, 6, 7, 15, 16, 64)] == [1, 1, 2, 2, 2, 2]
    assert [plan(lib, n, np.float32, s, 1, layout=0)["ns"] for s in (6, 7, 15, 16)] == [1, 1, 1, 2]
    assert [plan(lib, n, np.float32, s, 1, weno=1)["ns"] for s in (7, 64)] == [1, 1]
    assert [plan(lib, n, np.float32, 4, b)["skip"] for b in (1, 2, 4)] == [1, 1, 1]
    assert [plan(lib, n, np.float32, 4, b, opts={"probe_skip": 0})["skip"] for b in (1, 2, 4)] == [0, 1, 1]
    assert [plan(lib, (256, 256, 256), np.float64, 8, b)["skip"] for b in (1, 3, 4)] == [0, 0, 1]   # (fp64, 512 patches: no probe window)
    assert [plan(lib, (256, 256, 256), np.float32, 8, b)["skip"] for b in (1, 3, 4, 8)] == [0, 0, 1, 1]   # 256 patches: the window from 4 entries on
    assert [plan(lib, (256, 256, 256), np.float32, 8, b, opts={"probe_skip": 0})["skip"] for b in (3, 4, 7, 8)] == [0, 0, 0, 1]
    assert [plan(lib, n, np.float64, 5, b, layout=0)["chunk"] for b in (1, 4, 5)] == [16, 16, 8]   # f64_c16_below = 5 (32 x 64 patches: 5 slots in the window)
    assert [plan(lib, n, np.float32, 4, b, weno=1, stage=1)["chunk"] for b in (1, 2, 3)] == [16, 16, 8]   # weno_c16_below = 3
    env(TTCR_FSM_PAIR=1)
    assert [plan(lib, n, np.float32, 32, b, weno=1, stage=1)["chunk"] for b in (7, 8)] == [8, 4]   # weno_ch4_min = 8
    env(TTCR_FSM_SKIP_ALL_DIRTY=1, TTCR_FSM_PAIR=0)
    assert [plan(lib, n, np.float32, 4, b, opts={"probe_skip": 0})["skip"] for b in (1, 2)] == [0, 2]


def test_2d_rotated_template_does_not_skip(lib, env):
    env()
    assert plan(lib, (130, 65), np.float32, 3, 3, opts={"skip": 1})["skip"] == 1
    assert plan(lib, (130, 65), np.float32, 3, 3, opts={"skip": 1, "rotated": 1})["skip"] == 0
    assert plan(lib, (130, 65), np.float32, 3, 3, weno=1, stage=1, opts={"skip": 1, "rotated": 1})["skip"] == 1


# ---------------------------------------------------------------------------------------------------------------- the literals
def test_literal_plans(lib, env):
    env()
    n = (512, 512, 512)
    p = plan(lib, n, np.float32, 1, 1)
    assert p["name"] == "fsm_sweep_persistent<float,16,16,16,true,true,1,1,true,false>", p
    assert (p["status"], p["dyn_lds"], p["wgs"], p["block"], p["tickets"], p["launches"]) == (0, 0, 2048, 256, XS_BY_TIME, 1), p
    p = plan(lib, n, np.float32, 1, 1, opts={"lone_chunk": 8})
    assert p["name"] == "fsm_sweep_persistent<float,16,16,8,true,true,1,1,true,true>", p
    assert (p["status"], p["chunk"], p["pre"], p["dyn_lds"], p["wgs"]) == (0, 8, 1, 40000, 2048), p
    p = plan(lib, n, np.float32, 64, 32)
    assert p["name"] == "fsm_sweep_persistent<float,16,16,8,true,true,1,2,true,true>", p
    assert (p["status"], p["dyn_lds"], p["wgs"], p["ns"]) == (0, 0, 2048, 2), p
    p = plan(lib, (130, 65), np.float32, 16, 16)
    assert p["name"] == "fsm_sweep_persistent<float,64,1,16,false,true,1,1,true,true>", p
    assert (p["status"], p["dyn_lds"], p["wgs"], p["block"]) == (0, 0, 3 * 16 * 4, 64), p   # one workgroup per unit: 3 patches x 16 x 4
    # mode 0: one launch per tile wavefront; mode 1: one per sweep
    p = plan(lib, n, np.float32, 1, 1, opts={"mode": 0})
    assert p["name"] == "fsm_sweep_tile<float,16,16,16,true>" and p["status"] == 0 and p["launches"] % 8 == 0, p
    p = plan(lib, n, np.float32, 1, 1, opts={"mode": 1})
    assert p["name"] == "fsm_sweep_persistent<float,16,16,8,true,true,1,1,false,false>" and (p["wgs"], p["launches"], p["tickets"]) == (1024, 8, PER_SWEEP), p
    p = plan(lib, n, np.float32, 1, 1, opts={"arith": 1})
    assert p["name"] == "fsm_sweep_persistent<float,16,16,16,true,true,1,1,true,false,1>" and p["status"] == 0, p
    assert plan(lib, n, np.float32, 1, 1, opts={"arith": 1, "mode": 1})["status"] == 1


def test_argument_checks(lib, env):
    env()
    ok = dict(nodes=(37, 35, 41), dtype=np.float32, n_slots=3, batch=1)
    assert plan(lib, status_only=True, **ok) == 0
    for bad in (dict(batch=0), dict(batch=4), dict(n_slots=0), dict(stage=1), dict(nodes=(1, 35, 41)), dict(layout=2), dict(wg_cap=0),
                dict(opts={"lone_chunk": 4}), dict(opts={"arith": 3}), dict(opts={"no_such_option": 1})):
        assert plan(lib, status_only=True, **dict(ok, **bad)) != 0, bad
