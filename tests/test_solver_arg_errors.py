"""The argument errors of the field tape's solver, joint and receiver entries (ttcr_fsm_normal_*, ttcr_fsm_joint_*, ttcr_fsm_rjoint_*,
ttcr_fsm_rcv_*) that can be told with a NULL tape, replayed from tests/golden/solver_arg_errors.json: the table was recorded by
tests/golden/make_solver_arg_errors.py from the commit before these entries were put on one solve body, so status, message and the order
of the checks are held to what they were, not to what the code under test says.  Every case returns before any device call: no GPU is
needed."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_solver_arg_errors as M  # noqa: E402

with open(M.FIXTURE) as _f:
    _FIXTURE = json.load(_f)
TABLE = _FIXTURE["cases"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_the_table_covers_every_solver_entry():
    from ttcr_amd import _lib

    prefixes = ("ttcr_fsm_normal_", "ttcr_fsm_joint_", "ttcr_fsm_rjoint_", "ttcr_fsm_rcv_")
    entries = {n for n in _lib.SYMBOLS if n.startswith(prefixes)} - {"ttcr_fsm_normal_tile_edge"}   # (no tape, no error: it takes a dtype)
    assert entries == set(M.VALID) == {row["entry"] for row in TABLE} and len(entries) == 16
    # the table is the generator's list of cases, none dropped, and names the commit it was recorded from
    assert [(row["entry"], row["args"]) for row in TABLE] == [(e, a) for e, a in M.cases()]
    assert len(_FIXTURE["recorded_from"]) == 40
    messages = {row["message"] for row in TABLE} - {None}
    assert len(messages) == 35 and all(row["status"] == 1 and row["message"] for row in TABLE)   # (a NULL tape in every case)


def test_status_and_message_of_every_case(lib):
    from ttcr_amd import _lib

    bad = []
    for row in TABLE:
        got = M.call(lib, _lib.SYMBOLS, row["entry"], row["args"])
        if got != (row["status"], row["message"]):
            bad.append((row["entry"], row["args"], got, (row["status"], row["message"])))
    assert not bad, bad[:10]
