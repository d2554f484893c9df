"""The argument errors of the field tape's C entries (ttcr_fsm_adjoint_*) that can be told with a NULL tape, replayed from
tests/golden/field_tape_arg_errors.json: the table was recorded by tests/golden/make_field_tape_arg_errors.py from the commit before
the entries were put on one frame, so status, message and the order of the checks are held to what they were, not to what the code
under test says.  Every case returns before any device call: no GPU is needed."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_field_tape_arg_errors as M  # noqa: E402

with open(M.FIXTURE) as _f:
    TABLE = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def lib():
    from ttcr_amd import build, _lib

    build.build()
    return _lib.load()


def test_the_table_covers_every_entry_of_the_tape():
    from ttcr_amd import _lib

    tape_entries = {n for n in _lib.SYMBOLS if n.startswith("ttcr_fsm_adjoint_")}
    assert tape_entries == set(M.VALID) == {row["entry"] for row in TABLE}
    # the table is the generator's list of cases, none dropped
    assert [(row["entry"], row["args"]) for row in TABLE] == [(e, a) for e, a in M.cases()]
    messages = {row["message"] for row in TABLE} - {None}
    assert len(messages) == 12 and all(row["status"] == (0 if row["message"] is None else 1) for row in TABLE)


def test_status_and_message_of_every_case(lib):
    from ttcr_amd import _lib

    bad = []
    for row in TABLE:
        got = M.call(lib, _lib.SYMBOLS, row["entry"], row["args"])
        if got != (row["status"], row["message"]):
            bad.append((row["entry"], row["args"], got, (row["status"], row["message"])))
    assert not bad, bad[:10]
