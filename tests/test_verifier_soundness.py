"""Verifier soundness: forged proofs for the checks that a changed byte never reaches (CPU).

A proof with one byte changed no longer agrees with its own transcript, so it dies at a Merkle,
format or commitment check (or, inside the OOD frame, at the identity) and says nothing about the
checks behind those.  The oracle's dishonest prover (oracle.forge, or_forge) writes proofs that are
consistent with their transcript everywhere except at one place, so exactly one check of a verifier
can object: the OOD identity, the layer-0 fold comparison, a later fold comparison, the remainder
comparison, the proof of work.  Both verifiers (zk_verify of the library, or_verify of the oracle)
must reject each forgery with ZK_ERR_VERIFY / a nonzero status and with exactly that check's text,
taken from each verifier's own source: a rejection for another reason fails the test.

Inputs: the golden `lr` trace (n = 128).  The statement is made false either by one trace cell
(column 0, the clock, at row n/2) or by one asserted public value raised by 1 (outputs 0..7 and the
program hash are asserted; outputs 8..15 only enter the transcript seed).  Option sets, for both
field extensions: the default (no FRI layer), fold 4 / remainder degree 31 (one layer), fold 2 /
remainder degree 7 (four layers), and grinding 12 for the proof of work.

Also here: wrong public inputs at verify time, and one flipped bit at every byte offset of two honest
proofs through both verifiers (none accepted, every reason one of the verifier's own).
"""
import functools
import json
import re
import time
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from zkvm_amd import native
from zkvm_amd.prover import make_pub_inputs
from zkvm_amd.prover import verify as zk_verify

GOLD = Path(__file__).resolve().parent / "golden"
CASE = next(c for c in json.loads((GOLD / "cases.json").read_text())["cases"] if c["name"] == "lr")
HASH = [int(h, 16) for h in CASE["program_hash"]]
OUTS = [int(h, 16) for h in CASE["stack_outputs"]]
LWE, DELTA = CASE["lwe_size"], CASE["delta"]
N_ROWS = CASE["trace_len"]

# name -> (options that differ from the default, number of FRI layers at n = 128, blowup 8)
OPTION_SETS = {
    "nl0": ({}, 0),
    "nl1": ({"fri_folding": 4, "fri_rem_max_deg": 31}, 1),
    "nl4": ({"fri_folding": 2, "fri_rem_max_deg": 7}, 4),
    "grind12": ({"grinding": 12}, 0),
}

# each check's rejection text, from encrypt-zkvm_amd/csrc/verifier.cpp and from oracle/verifier.c
PRODUCT_TEXT = {"ood": "out-of-domain constraint evaluation mismatch", "fold": "FRI layer {l} folding mismatch",
                "rem": "FRI remainder mismatch", "pow": "query seed proof of work is invalid"}
ORACLE_TEXT = {"ood": "out-of-domain constraint evaluation mismatch", "fold": "FRI layer {l} folding mismatch",
               "rem": "FRI remainder mismatch", "pow": "query seed proof-of-work is invalid"}

# every reason either verifier can give (their sources' failure strings), for the exhaustive flips
_BATCH = r"(trace query|constraint query|FRI layer \d+ query)"
PRODUCT_REASONS = [
    "non-canonical field element", _BATCH + ": wrong number of paths", _BATCH + ": truncated path",
    _BATCH + ": malformed batch proof", _BATCH + ": missing sibling", _BATCH + ": path too short",
    _BATCH + " does not match the commitment", "malformed proof context", "field modulus mismatch",
    r"insufficient proof security: -?\d+", "malformed commitments", "expected one trace segment",
    "malformed out-of-domain frame", "out-of-domain constraint evaluation mismatch", "wrong number of FRI layers",
    "malformed proof tail", "remainder commitment mismatch", "query seed proof of work is invalid",
    "number of unique queries mismatch", "malformed query values", r"malformed FRI layer \d+",
    r"FRI layer \d+ folding mismatch", "remainder has the wrong size", "FRI remainder mismatch",
]
ORACLE_REASONS = [
    "malformed proof context", "field modulus mismatch", r"insufficient proof security: -?\d+ < \d+",
    "malformed commitments", "expected one trace segment", "malformed OOD frame", "non-canonical OOD value",
    "out-of-domain constraint evaluation mismatch", "wrong number of FRI layers", "malformed proof tail",
    "remainder commitment mismatch", "query seed proof-of-work is invalid", "number of unique queries mismatch",
    "malformed query values", "trace query does not match the commitment",
    "constraint query does not match the commitment", "non-canonical constraint value", r"malformed FRI layer \d+",
    r"non-canonical FRI value in layer \d+", r"FRI layer \d+ query does not match the commitment",
    r"FRI layer \d+ folding mismatch", "remainder has wrong size", "non-canonical remainder coefficient",
    "FRI remainder mismatch",
]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    """The conftest fixture rebuilds a stale liboracle.so before this module's first call."""


@functools.lru_cache(maxsize=None)
def valid_trace():
    t = np.load(GOLD / "lr.trace.npy", allow_pickle=False)
    assert t.shape == (28, N_ROWS, 2)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def invalid_trace():
    """The clock column at row n/2, low word XOR 1: transition constraint 0 fails on two rows."""
    t = valid_trace().copy()
    t[0, N_ROWS // 2, 0] ^= 1
    t.setflags(write=False)
    return t


def pubs(program_hash=HASH, outputs=OUTS, lwe_size=LWE, delta=DELTA):
    """The same public inputs for the oracle and for the library."""
    return (orc.make_pub(program_hash, outputs, lwe_size, delta),
            make_pub_inputs(program_hash, outputs, lwe_size, delta))


def raised(values, k):
    v = list(values)
    v[k] += 1
    return v


# a false statement: (trace, public inputs)
STATEMENTS = {
    "clock_cell": lambda: (invalid_trace(), pubs()),
    "out0": lambda: (valid_trace(), pubs(outputs=raised(OUTS, 0))),
    "out3": lambda: (valid_trace(), pubs(outputs=raised(OUTS, 3))),
    "out7": lambda: (valid_trace(), pubs(outputs=raised(OUTS, 7))),
    "hash0": lambda: (valid_trace(), pubs(program_hash=raised(HASH, 0))),
    "hash1": lambda: (valid_trace(), pubs(program_hash=raised(HASH, 1))),
}


def options(optset, ext):
    return orc.default_options(field_extension=ext, **OPTION_SETS[optset][0])


@functools.lru_cache(maxsize=None)
def honest(optset, ext):
    """The honest proof of the valid statement, checked once per (option set, extension): the forger's
    cheat = 0 run is or_prove byte for byte, and both verifiers accept it."""
    opub, zpub = pubs()
    proof, rec, _ = orc.prove(valid_trace(), opub, options(optset, ext))
    assert rec.num_fri_layers == OPTION_SETS[optset][1]
    forged, frec = orc.forge(valid_trace(), opub, options(optset, ext), orc.CHEAT_NONE)
    assert forged == proof and bytes(frec) == bytes(rec)
    assert orc.verify(proof, opub, 0) == (0, "")
    assert zk_verify(proof, zpub, 0) == (0, "")
    return proof


def forged_cases():
    """(id, extension, option set, cheat, arg, statement, check, layer) for every row of the cheat table."""
    out = []
    for ext in (1, 2):
        for optset in ("nl0", "nl1", "nl4"):
            nl = OPTION_SETS[optset][1]
            for stmt in STATEMENTS:
                out.append((ext, optset, "IGNORE_DEGREE", 0, stmt, "ood", None))
                out.append((ext, optset, "FIT_OOD", 0, stmt, "rem", None))
            out.append((ext, optset, "SHIFT_DEEP", 0, None, "fold" if nl else "rem", 0))
            for l in range(1, nl + 1):
                out.append((ext, optset, "BAD_FOLD", l, None, "fold" if l < nl else "rem", l))
        out.append((ext, "grind12", "NO_GRIND", 0, None, "pow", None))
    return [pytest.param(*c, id=f"ext{c[0]}-{c[1]}-{c[2]}{c[3] or ''}-{c[4] or 'valid'}") for c in out]


@pytest.mark.parametrize("ext,optset,cheat,arg,stmt,check,layer", forged_cases())
def test_forged_proof_dies_at_its_check(ext, optset, cheat, arg, stmt, check, layer):
    honest(optset, ext)
    trace, (opub, zpub) = STATEMENTS[stmt]() if stmt else (valid_trace(), pubs())
    opts = options(optset, ext)
    proof, rec = orc.forge(trace, opub, opts, getattr(orc, cheat), arg)
    assert proof and rec.num_fri_layers == OPTION_SETS[optset][1]
    if stmt:  # the statement is false: the honest prover refuses it
        assert orc.prove_rc(trace, opub, opts)[0] == -20
    else:
        assert proof != honest(optset, ext)
    if cheat == "NO_GRIND":
        assert rec.pow_nonce >= 1
    rc, why = zk_verify(proof, zpub, 0)
    assert (rc, why) == (native.ZK_ERR_VERIFY, PRODUCT_TEXT[check].format(l=layer))
    rc, why = orc.verify(proof, opub, 0)
    assert rc != 0 and why == ORACLE_TEXT[check].format(l=layer)


def test_forger_refuses_cheats_the_options_leave_no_room_for():
    opub, _ = pubs()
    for optset, cheat, arg in (("nl0", orc.BAD_FOLD, 1), ("nl4", orc.BAD_FOLD, 0), ("nl4", orc.BAD_FOLD, 5),
                               ("nl0", orc.NO_GRIND, 0), ("nl0", 6, 0)):
        with pytest.raises(orc.OracleError):
            orc.forge(valid_trace(), opub, options(optset, 1), cheat, arg)


# What the reference AIR leaves free: these are true statements for it, not forgeries.  A false statement
# above must not be swapped for one of them.
FREE_CELLS = [(13, N_ROWS // 2), (20, N_ROWS // 2), (27, N_ROWS // 2), (1, N_ROWS // 2), (7, N_ROWS // 2),
              (1, N_ROWS - 3), (7, N_ROWS - 3)]


@pytest.mark.parametrize("col,row", FREE_CELLS)
def test_cells_the_reference_air_leaves_free(col, row):
    t = valid_trace().copy()
    t[col, row, 0] ^= 1
    opub, zpub = pubs()
    rc, proof, _, _ = orc.prove_rc(t, opub, options("nl0", 1))
    assert rc == 0 and proof != honest("nl0", 1)
    assert orc.verify(proof, opub, 0) == (0, "") and zk_verify(proof, zpub, 0) == (0, "")


def test_outputs_past_the_eighth_are_not_asserted():
    """stack_outputs[8..15] enter the transcript seed and nothing else: a proof under a changed output 8
    is a valid proof of that statement."""
    opub, zpub = pubs(outputs=raised(OUTS, 8))
    rc, proof, _, _ = orc.prove_rc(valid_trace(), opub, options("nl0", 1))
    assert rc == 0 and proof != honest("nl0", 1)
    assert orc.verify(proof, opub, 0) == (0, "") and zk_verify(proof, zpub, 0) == (0, "")


WRONG_INPUTS = {
    "lwe4": dict(lwe_size=4), "lwe3": dict(lwe_size=3), "delta+1": dict(delta=DELTA + 1),
    "hash0": dict(program_hash=raised(HASH, 0)), "hash1": dict(program_hash=raised(HASH, 1)),
    "out0": dict(outputs=raised(OUTS, 0)), "out7": dict(outputs=raised(OUTS, 7)),
    "out8": dict(outputs=raised(OUTS, 8)), "out15": dict(outputs=raised(OUTS, 15)),
}


@pytest.mark.parametrize("ext", (1, 2))
@pytest.mark.parametrize("what", list(WRONG_INPUTS))
def test_honest_proof_under_wrong_inputs(what, ext):
    """An honest proof verified under other public inputs dies at the OOD identity: lwe_size and delta
    change the AIR side, the hash and the outputs (all sixteen) change the transcript."""
    proof = honest("nl0", ext)
    opub, zpub = pubs(**WRONG_INPUTS[what])
    assert zk_verify(proof, zpub, 0) == (native.ZK_ERR_VERIFY, PRODUCT_TEXT["ood"])
    rc, why = orc.verify(proof, opub, 0)
    assert rc != 0 and why == ORACLE_TEXT["ood"]


def sweep(verify, pub, proof, reasons):
    """One flipped bit (bit offset % 8) at every byte offset: (accepted offsets, histogram of the reasons,
    reasons that are not the verifier's own, seconds)."""
    known = [re.compile(r) for r in reasons]
    accepted, hist = [], Counter()
    bad = bytearray(proof)
    t0 = time.perf_counter()
    for off in range(len(proof)):
        bad[off] ^= 1 << (off % 8)
        rc, why = verify(bytes(bad), pub, 0)
        bad[off] = proof[off]
        if rc == 0:
            accepted.append(off)
        hist[why] += 1
    dt = time.perf_counter() - t0
    foreign = sorted(w for w in hist if not any(k.fullmatch(w) for k in known))
    return accepted, hist, foreign, dt


# (option set, extension): the default proof (29.7 KB) and the quadratic four-layer one (about 47 KB)
SWEEPS = [pytest.param("nl0", 1, id="default"), pytest.param("nl4", 2, id="quad_nl4", marks=pytest.mark.slow)]


@pytest.mark.parametrize("optset,ext", SWEEPS)
def test_every_offset_flipped_product(optset, ext):
    proof = honest(optset, ext)
    accepted, hist, foreign, dt = sweep(zk_verify, pubs()[1], proof, PRODUCT_REASONS)
    print(f"zk_verify, {len(proof)} B, {dt:.1f} s: {dict(hist.most_common())}")
    assert accepted == [] and foreign == [] and sum(hist.values()) == len(proof)


@pytest.mark.parametrize("optset,ext", SWEEPS)
def test_every_offset_flipped_oracle(optset, ext):
    proof = honest(optset, ext)
    accepted, hist, foreign, dt = sweep(orc.verify, pubs()[0], proof, ORACLE_REASONS)
    print(f"or_verify, {len(proof)} B, {dt:.1f} s: {dict(hist.most_common())}")
    assert accepted == [] and foreign == [] and sum(hist.values()) == len(proof)
