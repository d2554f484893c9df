"""Records tests/golden/field_tape_arg_errors.json: what every product entry and getter of the field tape (ttcr_fsm_adjoint_*,
include/ttcr_amd.h) answers to an argument error that can be told with a NULL tape -- status and the full message of
ttcr_fsm_last_error.  All of these return before any device call, so no GPU is needed.

Run it in a checkout of the commit whose answers are to be pinned (tests/test_field_tape_arg_errors.py replays the table against the
build at hand, so a table recorded from that same build would pin nothing):

    python tests/golden/make_field_tape_arg_errors.py [--commit NAME]

An argument of a case is a small integer, "null" or "ptr" (a valid pointer to 128 zero bytes).  The one-vector entries check the tape
first, so "null tape" is all they can say here; their cases vary everything else to hold that order.  The block entries check the tape
last: each of their errors is reached by making everything checked before it valid.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "field_tape_arg_errors.json")

N, P = "null", "ptr"
# entry -> a call with a NULL tape and everything else valid (n_cols 3 for the block entries)
VALID = {
    "ttcr_fsm_adjoint_model": [N, P, P, P],
    "ttcr_fsm_adjoint_size": [N, P, P, P],
    "ttcr_fsm_adjoint_bytes": [N, P],
    "ttcr_fsm_adjoint_device": [N, P],
    "ttcr_fsm_adjoint_get_field": [N, 0, P],
    "ttcr_fsm_adjoint_points": [N, P, P],
    "ttcr_fsm_adjoint_vjp": [N, P, 0, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_jvp": [N, P, 0, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_gn": [N, P, 0, P, 0, P, 0, 0, P, P],
    "ttcr_fsm_adjoint_jvp_source": [N, P, 0, 2, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_vjp_source": [N, P, 0, P, 0, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_hold": [N, P, 0, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_release": [N],
    "ttcr_fsm_adjoint_hvp": [N, P, 0, P, 0, 0, P, P],
    "ttcr_fsm_adjoint_newton": [N, P, 0, P, 0, P, 0, 0, P, P],
    "ttcr_fsm_adjoint_jvp_block": [N, 3, P, 0, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_vjp_block": [N, 3, P, 0, P, 0, 0, P],
    "ttcr_fsm_adjoint_gn_block": [N, 3, P, 0, P, 3, 0, P, 0, 0, P, P],
    "ttcr_fsm_adjoint_block_release": [N],
    "ttcr_fsm_adjoint_free": [N],
}
# position of the schedule (and of the column count, where there is one) in the argument list
SCHEDULE = {"ttcr_fsm_adjoint_vjp": 7, "ttcr_fsm_adjoint_jvp": 7, "ttcr_fsm_adjoint_gn": 7, "ttcr_fsm_adjoint_jvp_source": 8,
            "ttcr_fsm_adjoint_vjp_source": 9, "ttcr_fsm_adjoint_hold": 7, "ttcr_fsm_adjoint_hvp": 5, "ttcr_fsm_adjoint_newton": 7,
            "ttcr_fsm_adjoint_jvp_block": 8, "ttcr_fsm_adjoint_vjp_block": 6, "ttcr_fsm_adjoint_gn_block": 9}
N_COLS = {"ttcr_fsm_adjoint_jvp_source": 3, "ttcr_fsm_adjoint_jvp_block": 1, "ttcr_fsm_adjoint_vjp_block": 1,
          "ttcr_fsm_adjoint_gn_block": 1}


def _with(args, **at):
    out = list(args)
    for i, v in at.items():
        out[int(i[1:])] = v
    return out


def cases():
    """every (entry, arguments) of the table, in a fixed order"""
    out = []
    for entry, valid in VALID.items():
        rows = [valid]
        # every pointer in turn NULL, then all of them; every on-device flag 1
        ptrs = [i for i, a in enumerate(valid) if a == P]
        rows += [_with(valid, **{"a%d" % i: N}) for i in ptrs]
        if len(ptrs) > 1:
            rows.append([N if a == P else a for a in valid])
        if entry in SCHEDULE:
            rows += [_with(valid, **{"a%d" % SCHEDULE[entry]: s}) for s in (1, 2, -1)]
        if entry in N_COLS:
            rows += [_with(valid, **{"a%d" % N_COLS[entry]: k}) for k in (0, -3, 1, 4, 5, 9)]
        out += [(entry, r) for r in rows]
    # the block entries check the tape last: combinations that reach the later checks with the earlier ones valid or not
    jb, vb, gb = "ttcr_fsm_adjoint_jvp_block", "ttcr_fsm_adjoint_vjp_block", "ttcr_fsm_adjoint_gn_block"
    out += [(jb, _with(VALID[jb], a1=0, a8=2)), (jb, _with(VALID[jb], a8=2, a2=N)), (jb, _with(VALID[jb], a2=N, a4=N, a6=N)),
            (jb, _with(VALID[jb], a4=N, a6=N)), (jb, _with(VALID[jb], a4=N)), (jb, _with(VALID[jb], a6=N, a8=1, a1=5))]
    out += [(vb, _with(VALID[vb], a1=0, a6=2)), (vb, _with(VALID[vb], a6=2, a2=N)), (vb, _with(VALID[vb], a2=N, a4=N)),
            (vb, _with(VALID[vb], a6=1, a1=5))]
    for rw_cols in (-1, 0, 1, 2, 3, 4):   # (n_cols = 3)
        out += [(gb, _with(VALID[gb], a5=rw_cols)), (gb, _with(VALID[gb], a5=rw_cols, a4=N)), (gb, _with(VALID[gb], a5=rw_cols, a9=2)),
                (gb, _with(VALID[gb], a5=rw_cols, a2=N)), (gb, _with(VALID[gb], a5=rw_cols, a7=N)), (gb, _with(VALID[gb], a5=rw_cols, a1=0)),
                (gb, _with(VALID[gb], a5=rw_cols, a4=N, a1=0))]
    out += [(gb, _with(VALID[gb], a1=0, a9=2)), (gb, _with(VALID[gb], a9=2, a2=N)), (gb, _with(VALID[gb], a2=N, a7=N)),
            (gb, _with(VALID[gb], a1=1, a5=1)), (gb, _with(VALID[gb], a1=1, a5=3))]
    return out


def call(lib, symbols, entry, args):
    """(status, message or None) of one case: the message is read only after a failure (a success leaves the last one standing)"""
    keep = []
    real = []
    for ty, a in zip(symbols[entry][1], args):
        if a == N:
            real.append(None)
        elif a == P:
            keep.append((C.c_double * 16)())
            real.append(C.cast(keep[-1], ty))
        else:
            real.append(int(a))
    assert len(real) == len(symbols[entry][1]), entry
    status = getattr(lib, entry)(*real)
    assert all(not any(b) for b in keep), (entry, args)   # (no case gets as far as its outputs)
    return int(status), (lib.ttcr_fsm_last_error().decode() if status != 0 else None)


def main():
    sys.path.insert(0, ROOT)
    from ttcr_amd import _lib, build

    build.build()
    lib = _lib.load()
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None
    table = []
    for entry, args in cases():
        status, message = call(lib, _lib.SYMBOLS, entry, args)
        table.append({"entry": entry, "args": args, "status": status, "message": message})
    with open(FIXTURE, "w") as f:
        f.write('{"recorded_from": %s,\n "cases": [\n' % json.dumps(commit))
        f.write(",\n".join("  " + json.dumps(row) for row in table))
        f.write("\n]}\n")
    print("%d cases -> %s" % (len(table), FIXTURE))


if __name__ == "__main__":
    main()
