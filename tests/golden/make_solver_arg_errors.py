"""Records tests/golden/solver_arg_errors.json: what the solver, joint and receiver entries of the field tape (ttcr_fsm_normal_*,
ttcr_fsm_joint_*, ttcr_fsm_rjoint_*, ttcr_fsm_rcv_*, include/ttcr_amd.h) answer to an argument error that can be told with a NULL tape
-- status and the full message of ttcr_fsm_last_error.  These entries check the tape last, so every check before it is reached by making
what is checked earlier valid; all of them return before any device call, so no GPU is needed.

Run it in a checkout of the commit whose answers are to be pinned (tests/test_solver_arg_errors.py replays the table against the build
at hand, so a table recorded from that same build would pin nothing):

    python tests/golden/make_solver_arg_errors.py [--commit NAME]

An argument of a case is an integer, a float ("nan" and "inf" as strings), "null", "ptr" (a valid pointer to 128 zero bytes: three
smoothing weights of 0 where weights are read) or a list of three such floats (smoothing weights).  Per entry: the valid call, every
pointer NULL in turn and all of them at once, every scalar setting bad in turn (negative, NaN, infinite, maxiter 0 and -1, hessian 2 and
-1, schedule 2 and -1, a negative, a NaN and an infinite smoothing weight), and every pair of these faults in two different arguments,
which fixes the order of the checks.

What this table cannot reach are the checks behind the tape: the values of the scale and damping of a block, the rule of three
parameters per axis for a smoothing term, the event indices of rcv_eval and the point indices of rcv_points.  The GPU tests of the
Python layer (tests/test_normal_solve_gpu.py, tests/test_joint_solve_gpu.py, tests/test_receiver_derivative_gpu.py) hold those.
"""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "solver_arg_errors.json")

N, P = "null", "ptr"
_JVP = [N, P, 0, P, 0, P, 0, P, 0, 0, P]
_GN = [N, P, 0, P, 0, P, 0, P, P, 0, P, 0, 0, P, P]
_SOLVE = [N, P, 0, P, 0, P, 0, 1.0, [1.0, 1.0, 1.0], 0.5, P, P, 5, 1e-6, 0, P, 0, P, 0, P, P, P, P, P]
# entry -> a call with a NULL tape and everything else valid
VALID = {
    "ttcr_fsm_normal_smooth": [N, P, 0, [1.0, 1.0, 1.0], P, 0],
    "ttcr_fsm_normal_dot": [N, P, 0, P, 0, P],
    "ttcr_fsm_normal_solve": [N, P, 0, P, 0, 1.0, [1.0, 1.0, 1.0], 0.5, P, 0, 5, 1e-6, 0, 0, P, 0, P, P, P, P, P],
    "ttcr_fsm_normal_release": [N],
    "ttcr_fsm_joint_jvp": _JVP,
    "ttcr_fsm_joint_gn": _GN,
    "ttcr_fsm_joint_solve": _SOLVE,
    "ttcr_fsm_joint_release": [N],
    "ttcr_fsm_rjoint_jvp": _JVP,
    "ttcr_fsm_rjoint_gn": _GN,
    "ttcr_fsm_rjoint_solve": _SOLVE,
    "ttcr_fsm_rcv_eval": [N, 2, P, 0, P, P, 0, P, 0],
    "ttcr_fsm_rcv_points": [N, P, 2, P, P, P],
    "ttcr_fsm_rcv_jvp": [N, P, 0, P, 0],
    "ttcr_fsm_rcv_vjp": [N, P, 0, P, 0],
    "ttcr_fsm_rcv_release": [N],
}
# positions of the settings in the argument lists: finite values >= 0, the smoothing weights, maxiter, hessian, schedule
_SOLVE_SETTINGS = {"nonneg": [7, 9, 13], "weights": 8, "maxiter": 12, "schedule": 14}
SETTINGS = {
    "ttcr_fsm_normal_smooth": {"weights": 3},
    "ttcr_fsm_normal_solve": {"nonneg": [5, 7, 11], "weights": 6, "maxiter": 10, "hessian": 12, "schedule": 13},
    "ttcr_fsm_joint_jvp": {"schedule": 9},
    "ttcr_fsm_joint_gn": {"schedule": 12},
    "ttcr_fsm_joint_solve": _SOLVE_SETTINGS,
    "ttcr_fsm_rjoint_jvp": {"schedule": 9},
    "ttcr_fsm_rjoint_gn": {"schedule": 12},
    "ttcr_fsm_rjoint_solve": _SOLVE_SETTINGS,
}


def faults(entry):
    """every (position, bad value) of an entry, in a fixed order"""
    valid = VALID[entry]
    out = [(i, N) for i, a in enumerate(valid) if a == P or isinstance(a, list)]
    st = SETTINGS.get(entry, {})
    for i in st.get("nonneg", []):
        out += [(i, -1.0), (i, "nan"), (i, "inf")]
    if "weights" in st:
        out += [(st["weights"], w) for w in ([1.0, 1.0, -1.0], ["nan", 1.0, 1.0], [1.0, "inf", 1.0])]
    if "maxiter" in st:
        out += [(st["maxiter"], 0), (st["maxiter"], -1)]
    if "hessian" in st:
        out += [(st["hessian"], 2), (st["hessian"], -1)]
    if "schedule" in st:
        out += [(st["schedule"], 2), (st["schedule"], -1)]
    return out


def _with(args, *changes):
    out = list(args)
    for i, v in changes:
        out[i] = v
    return out


def cases():
    """every (entry, arguments) of the table, in a fixed order"""
    out = []
    for entry, valid in VALID.items():
        fs = faults(entry)
        rows = [valid] + [_with(valid, f) for f in fs]
        ptrs = [f for f in fs if f[1] == N]
        if len(ptrs) > 1:
            rows.append(_with(valid, *ptrs))
        st = SETTINGS.get(entry, {})
        if "schedule" in st:
            rows.append(_with(valid, (st["schedule"], 1)))
        if "hessian" in st:
            rows.append(_with(valid, (st["hessian"], 1)))
        first = [next(f for f in fs if f[0] == i) for i in sorted({f[0] for f in fs})]   # (one fault per argument)
        rows += [_with(valid, f, g) for f, g in itertools.combinations(first, 2)]
        out += [(entry, r) for r in rows]
    return out


def _float(a):
    return float(a)   # ("nan" and "inf" too)


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
        elif isinstance(a, list):
            real.append((C.c_double * 3)(*[_float(v) for v in a]))
        elif ty is C.c_double:
            real.append(_float(a))
        else:
            real.append(int(a))
    assert len(real) == len(symbols[entry][1]) == len(args), entry
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
