"""What tests/test_change_sum_gpu.py relies on, checked on the CPU with the oracle alone (tests/change_sum_cases.py): every case has
iterations to compare, the exact decreases are exact (no node goes up, every long-double difference is exact and fits a float64), and the
oracle's own `change` -- the reference's sequential sum in the grid's precision -- lies within gamma = N u / (1 - N u) of the exact
decrease: the exact sum reached by an independent route."""
import math

import numpy as np
import pytest

import change_sum_cases as cs
import few_workgroups_cases as fw


@pytest.mark.parametrize("name,dt", cs.ROWS, ids=cs.ROW_IDS)
def test_exact_decrease_against_the_oracles_sum(oracle, name, dt):
    c = cs.BY_NAME[name]
    g = cs.gamma(dt, cs.n_nodes(c))
    worst = 0.0
    for q in range(c["n_src"]):
        f = cs.fields(oracle, c, dt, q)          # (asserts of exact_decrease and fields run here)
        K = f["niter"]
        assert len(f["F"]) == K + 1 and len(f["E"]) == K + 1 and f["change"].size == K
        if c["rotated"]:
            assert K == cs.K_ROT                 # the rough model does not let the rotated template converge: every iteration is compared
        else:
            assert K < cs.MAXIT                  # the stopping rule ended the solve
        positive = [k for k in range(2, K + 1) if f["E"][k] > 0]
        assert len(positive) >= (1 if c["nodes"] == (2, 16, 10) else 2), (name, dt.name, q, f["E"])
        for k in range(2, K + 1):
            E, s = f["E"][k], float(f["change"][k - 1])
            assert E >= 0 and math.isfinite(E)
            if E == 0:
                assert s == 0
            else:
                worst = max(worst, abs(s / E - 1) / g)
                assert abs(s / E - 1) <= g, (name, dt.name, q, k, s, E, g)
    print(name, dt.name, "oracle sum against the exact decrease: worst |s / E - 1| / gamma", worst)


def test_exact_decrease():
    a = np.array([3.0, 2.5, 1.0 + 2.0 ** -23, 7.0], dtype=np.float32)
    b = np.array([3.0, 1.25, 1.0, 2.0 ** -20], dtype=np.float32)
    assert cs.exact_decrease(a, b) == 1.25 + 2.0 ** -23 + (7.0 - 2.0 ** -20)
    # a million terms a sequential fp32 sum would lose
    big = np.full(1 << 20, 1.0 + 2.0 ** -23, dtype=np.float32)
    big[0] = 2.0 ** 20
    low = np.ones(1 << 20, dtype=np.float32)
    assert cs.exact_decrease(big, low) == (2.0 ** 20 - 1.0) + ((1 << 20) - 1) * 2.0 ** -23
    with pytest.raises(AssertionError):
        cs.exact_decrease(b, a)                  # a node went up
    with pytest.raises(AssertionError):          # 1 - 2^-70 needs 70 bits
        cs.exact_decrease(np.array([1.0]), np.array([2.0 ** -70]))


def test_bar_restates_the_hosts_bound():
    u32, u64 = 2.0 ** -24, 2.0 ** -53
    assert cs.bar(np.float32, (37, 35, 41)) == 2.0 * (37 + 35 + 41 + 64) * u32 + 1e-6
    assert cs.bar(np.float32, (8192, 64)) == 2.0 * (64 + 8192 + 1 + 64) * u32 + 1e-6
    assert cs.geom((65, 130)) == (130, 65, 1)
    n = 37 * 35 * 41
    assert cs.bar(np.float64, (37, 35, 41)) == 1e-6 - n * u64 / (1 - n * u64) < 1e-6
    # the text of the bound in the host code
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ttcr_amd", "csrc", "fsm_capi.hip")).read()
    assert "m = 2.0 * (double)(geom.NF + geom.NJ + geom.NK + 64) * u + 1e-6" in src
    assert "geom.NF = nz + 1; geom.NJ = nx + 1; geom.NK = 1;" in src
    assert "window_lo() const { return sizeof(T) == 4 ? 0.5 : 1.0 - 1e-6; }" in src


def test_case_table():
    names = [c["name"] for c in cs.CASES]
    assert names[:4] == ["fw_" + "x".join(map(str, s)) for s in fw.SHAPES]
    for n in ("cells_21x20x24", "cells2d_131x67", "n2d_65x130", "n2d_130x65", "rot_1201x150", "rot_8192x64", "rot_64x8192", "rot_2051x40"):
        assert n in cs.BY_NAME
    c = cs.BY_NAME["n2d_65x130"]
    assert (c["dx"], c["dz"]) == (0.2, 0.3) and c["nodes"][0] % 64 == 1      # (patches of 64 columns along x: remainders 1 ...
    c = cs.BY_NAME["n2d_130x65"]
    assert c["dx"] == c["dz"] and c["nodes"][0] % 64 == 2                    # ... and 2)
    for c in cs.CASES:
        if c["rotated"]:
            assert c["dx"] == c["dz"] == 0.25 and c["maxit"] == cs.K_ROT and not c["cell"]
            assert cs.n_nodes(c) <= 524288
            s = cs.slowness(c, np.float32)
            assert s.shape == c["nodes"] and 0.25 <= s.min() and s.max() < 1.0
        src = cs.sources(c)
        ax = cs.axes(c, np.float64)
        assert src.shape == (c["n_src"], c["dim"])
        for d in range(c["dim"]):
            assert np.all(src[:, d] > ax[d][0]) and np.all(src[:, d] < ax[d][-1])
            h = ax[d][1] - ax[d][0]
            r = (src[:, d] - ax[d][0]) / h
            assert c["kind"] == "fw" or np.all(np.abs(r - np.round(r)) > 1e-3)   # off the node planes (fw: its own table, one source on a node)
    assert cs.BY_NAME["rot_1201x150"]["dtypes"] == (np.dtype(np.float32), np.dtype(np.float64))
    assert 1201 > 1022 + 1                       # (the strip kernel's fp32 strips hold 1022 columns)
