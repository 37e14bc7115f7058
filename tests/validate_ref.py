"""Reference trace validator for the tests of zk_validate_device / zk_validate_columns.

winterfell 0.9's Trace::validate, restated over the CPU oracle's ProcessorAir (oracle.periodic_row,
oracle.eval_transition -- here through the C functions those two wrap, fed the trace's own bytes): every assertion of
get_assertions against the trace, then evaluate_transition at every step 0 .. n - 3 with the periodic values of row
s mod 16.  reference_report builds the fields of zk_validation (include/zkvm_gpu.h) as native.Validation.to_dict()
returns them, and reference_message the text zk_last_error() carries for a failing trace.
"""
import ctypes as C

import numpy as np

NUM_TCONS, NUM_ASSERTS = 20, 22
U64_MAX = 2**64 - 1
ZK_OK, ZK_ERR_TRACE = 0, -21


def _el(b, k=0):
    return int.from_bytes(b[16 * k:16 * k + 16], "little")


def assertions(n, pub):
    """get_assertions (air/src/lib.rs:170-195) in its own order: (column, step, value)."""
    ph, so = bytes(pub.program_hash), bytes(pub.stack_outputs)
    a = [(0, 0, 0), (11, 0, 0)]
    for i in range(2):
        a += [(7 + i, 0, 0), (7 + i, n - 2, _el(ph, i))]
    for i in range(8):
        a += [(12 + i, 0, 0), (12 + i, n - 2, _el(so, i))]
    return a


class StepEvaluator:
    """evaluate_transition at single steps of one trace ((28, n, 2) uint64), through the oracle."""

    def __init__(self, oracle, trace, pub):
        self.fn = oracle.lib().or_air_eval_transition
        self.rows = np.ascontiguousarray(np.asarray(trace, dtype=np.uint64).transpose(1, 0, 2))  # (n, 28, 2)
        self.n = self.rows.shape[0]
        self.lwe_size, self.delta = pub.lwe_size, pub.delta
        self.per = []
        for r in range(16):
            want = oracle.periodic_row(r)
            assert len(want) == 9
            self.per.append(b"".join(int(v).to_bytes(16, "little") for v in want))
        self.out = C.create_string_buffer(16 * NUM_TCONS)

    def __call__(self, s):
        """The 20 constraint values of the frame (s, s + 1)."""
        self.fn(self.rows[s].tobytes(), self.rows[s + 1].tobytes(), self.per[s % 16], self.lwe_size, self.delta, self.out)
        raw = self.out.raw
        return [_el(raw, k) for k in range(NUM_TCONS)]


def reference_report(oracle, trace, pub, steps=None):
    """The zk_validation of `trace` as a dict.  steps: the steps to evaluate (default: all of 0 .. n - 3); a caller
    that knows every other step holds (the trace is a valid one changed in a few cells) passes the steps next to
    the changed cells."""
    trace = np.asarray(trace, dtype=np.uint64)
    n = trace.shape[1]
    ev = StepEvaluator(oracle, trace, pub)
    rep = {"trace_len": n, "steps_checked": n - 2, "failing_steps": 0,
           "t_count": [0] * NUM_TCONS, "t_first": [U64_MAX] * NUM_TCONS, "t_value": [0] * NUM_TCONS,
           "a_failed": 0, "a_mask": 0, "a_col": [], "a_step": [], "a_expected": [], "a_found": [],
           "first_kind": 0, "first_index": -1, "first_step": 0}
    for k, (col, step, value) in enumerate(assertions(n, pub)):
        found = int(trace[col, step, 0]) | (int(trace[col, step, 1]) << 64)
        rep["a_col"].append(col)
        rep["a_step"].append(step)
        rep["a_expected"].append(value)
        rep["a_found"].append(found)
        if found != value:
            rep["a_mask"] |= 1 << k
            rep["a_failed"] += 1
    todo = range(n - 2) if steps is None else sorted(set(s for s in steps if 0 <= s < n - 2))
    for s in todo:
        vals = ev(s)
        if any(vals):
            rep["failing_steps"] += 1
            for k, v in enumerate(vals):
                if v:
                    rep["t_count"][k] += 1
                    if rep["t_first"][k] == U64_MAX:
                        rep["t_first"][k], rep["t_value"][k] = s, v
    if rep["a_mask"]:
        k = (rep["a_mask"] & -rep["a_mask"]).bit_length() - 1
        rep["first_kind"], rep["first_index"], rep["first_step"] = 1, k, rep["a_step"][k]
    elif rep["failing_steps"]:
        s = min(rep["t_first"])
        rep["first_kind"], rep["first_index"], rep["first_step"] = 2, rep["t_first"].index(s), s
    return rep


def reference_rc(rep):
    return ZK_OK if rep["first_kind"] == 0 else ZK_ERR_TRACE


def reference_message(rep):
    """zk_last_error() after a failing validation: the first failure in winterfell's wording, then the totals."""
    k = rep["first_index"]
    if rep["first_kind"] == 1:
        head = f"trace does not satisfy assertion main_trace({rep['a_col'][k]}, {rep['a_step'][k]}) == {rep['a_expected'][k]}"
    else:
        head = f"main transition constraint {k} did not evaluate to ZERO at step {rep['first_step']}"
    return f"{head}; {rep['failing_steps']} failing steps, {rep['a_failed']} failed assertions"


def add_to_cell(trace, col, row, delta):
    """A copy of the trace with cell (col, row) := cell + delta mod p."""
    p = 2**128 - 45 * 2**40 + 1
    t = np.array(trace, dtype=np.uint64, copy=True)
    v = (int(t[col, row, 0]) | (int(t[col, row, 1]) << 64)) + delta
    v %= p
    t[col, row, 0], t[col, row, 1] = v & (2**64 - 1), v >> 64
    return t


def neighbour_steps(rows):
    """The steps whose frame (s, s + 1) holds one of `rows`."""
    return sorted({s for r in rows for s in (r - 1, r) if s >= 0})
