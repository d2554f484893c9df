"""What tests/test_few_workgroups_gpu.py relies on, checked on the CPU so that it cannot silently stop holding (tests/few_workgroups_cases.py):
the solves are long enough for every hand-over of state between launches, and the sources of a batch converge at different iterations, so
that the kernels meet converged batch entries (grp < 0) and partly converged pairs (lmask)."""
import numpy as np
import pytest

import few_workgroups_cases as fw

# iterations of the four sources, both precisions (measured with the oracle; the GPU tests assert the oracle's count, whatever it is)
NITER = {(37, 35, 41): [4, 4, 4, 4], (19, 50, 36): [4, 4, 5, 4], (70, 17, 9): [4, 4, 5, 5], (2, 16, 10): [2, 2, 3, 3]}


def _niter(oracle, shape, dtype):
    return [fw.reference(oracle, shape, dtype, k)["niter"] for k in range(fw.N_SRC)]


@pytest.mark.parametrize("dtype", fw.DTYPES, ids=["fp32", "fp64"])
def test_iteration_counts(oracle, dtype):
    for shape in fw.SHAPES:
        n = _niter(oracle, shape, dtype)
        assert n == NITER[shape], (shape, n)
        if shape in fw.LARGER:
            assert min(n) >= 4, (shape, n)           # several launches per solve: every counter and epoch word is reused
        assert max(n) < 50                           # (the stopping rule ended every solve, not maxit)


@pytest.mark.parametrize("dtype", fw.DTYPES, ids=["fp32", "fp64"])
def test_batches_hold_sources_that_converge_at_different_iterations(oracle, dtype):
    mixed = 0
    for shape in fw.SHAPES:
        n = _niter(oracle, shape, dtype)
        for order in (list(range(fw.N_SRC)), list(range(fw.N_SRC))[::-1]):
            for n_threads in (2, 3, 4):
                _, rounds = fw.held(order, n_threads)
                mixed += sum(len({n[k] for k in r}) > 1 for r in rounds)
    assert mixed >= 12, mixed
    # every shape but the first has such a batch with three and with four slots
    for shape in fw.SHAPES[1:]:
        n = _niter(oracle, shape, dtype)
        for n_threads in (3, 4):
            assert any(len({n[k] for k in r}) > 1 for r in fw.held(list(range(fw.N_SRC)), n_threads)[1]), (shape, n_threads)


@pytest.mark.parametrize("dtype", fw.DTYPES, ids=["fp32", "fp64"])
def test_a_pair_holds_sources_of_different_iteration_counts(oracle, dtype):
    """(70, 17, 9), four slots, option pair_sources = 0: the pairs are the (first, second) and (third, fourth) source of the call"""
    n = _niter(oracle, (70, 17, 9), dtype)
    for order in (fw.PAIR_ORDER_70, fw.PAIR_ORDER_70[::-1]):
        pairs = [(order[0], order[1]), (order[2], order[3])]
        assert sorted(sorted(n[k] for k in p) for p in pairs) == [[4, 5], [4, 5]], (order, n)


def test_held_sources():
    assert fw.held([0, 1, 2, 3], 3) == ({0: 1, 1: 2, 2: 3}, [[0, 2, 3], [1]])
    assert fw.held([3, 2, 1, 0], 3) == ({0: 2, 1: 1, 2: 0}, [[3, 1, 0], [2]])
    assert fw.held([0, 1, 2, 3], 2) == ({0: 1, 1: 3}, [[0, 2], [1, 3]])
    assert fw.held([0, 1, 2, 3], 4) == ({0: 0, 1: 1, 2: 2, 3: 3}, [[0, 1, 2, 3]])
    assert fw.held([0, 1, 2, 3], 1) == ({0: 3}, [[0], [1], [2], [3]])


def test_inputs():
    for shape in fw.SHAPES:
        for dtype in fw.DTYPES:
            s = fw.slowness(shape, dtype)
            assert s.shape == shape and s.dtype == dtype and 0.25 <= s.min() and s.max() <= 1.0
        src, rcv = fw.sources(shape), fw.receivers(shape)
        hi = np.array([(m - 1) * fw.DX for m in shape])
        assert src.shape == (4, 3) and np.all(src > 0) and np.all(src < hi)
        assert np.all(rcv >= 0) and np.all(rcv <= hi) and len(rcv) >= 5
        # corners, and a point off every node plane
        assert np.any(np.all(rcv == 0, axis=1)) and np.any(np.all(rcv == hi, axis=1))
        assert np.any(np.all(np.abs(rcv / fw.DX - np.round(rcv / fw.DX)) > 0.1, axis=1))
    assert sorted(fw.SHAPES[0]) == [35, 37, 41] and np.prod(fw.SHAPES[0]) < 60000
