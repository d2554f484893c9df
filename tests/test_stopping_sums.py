"""The CPU side of tests/test_stopping_sums_gpu.py, against the oracle alone: every case of the table has the targets the device test
counts on, and for each of them the second solve ends its stage at the targeted iteration with a `change` below eps * N and inside the
window in which the device decides by the reference's own sum (stopping_sums_cases.aim asserts that)."""
import numpy as np
import pytest

import stopping_sums_cases as sc

ALL = [(c, dt) for c in sc.CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("c,dt", ALL, ids=[f"{c['name']}-{dt.name}" for c, dt in ALL])
def test_every_target_is_decided_by_the_reference_sum(oracle, c, dt):
    ks = sc.targets(oracle, c, dt)
    print(c["name"], dt.name, "history", sc.history(c, sc.solve(oracle, c, dt, 0, 1e-9)), "targets", ks)
    want = {"odd_37x29x45": 3, "cells_21x20x24": 2, "n2d_151x71": 6, "weno_25x27x23": 3, "weno_cells2d_131x67": 3, "big_97x83x91": 2}
    assert len(ks) >= want.get(c["name"], 2), ks
    if c["weno"]:
        assert ks[0] == 0
    else:
        assert ks[0] == 1
    for k in ks:
        eps, thr, o2 = sc.aim(oracle, c, dt, k)
        assert eps > 0 and np.isfinite(o2["tt"]).all()


def test_the_shapes_take_the_paths_they_are_meant_for():
    """the arithmetic behind the case table: vector widths, block and brick remainders"""
    n = {c["name"]: sc.n_nodes(c) for c in sc.CASES}
    assert n["odd_37x29x45"] % 2 == 1 and n["vec_36x29x45"] % 4 == 0 and 36 % 4 == 0
    assert n["vec_34x30x46"] % 4 == 0 and 34 % 4 == 2 and n["n4r2_38x29x45"] % 4 == 2
    assert n["big_97x83x91"] == 732641 and -(-n["big_97x83x91"] // 4096) == 179
    for c in sc.CASES:
        assert n[c["name"]] % 4096 != 0 and any(v % 16 for v in c["nodes"])
