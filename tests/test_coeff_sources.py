"""Derived columns' coefficients read at their source by the boundary quotient, OOD and DEEP stages (zk_internal.hpp
CoeffSrc).

From a prover's third proof of a (trace length, program) the derived clock, the fixed columns and the hinted sparse
columns are each base_c + w_c e_(n-1); the host-trace path no longer writes those sums into the coefficient buffer: the
three stages that are linear in the trace polynomials read base_c and e_(n-1) where they lie and fold the scalars in.

  - whole proofs at 2^13 (the smallest length with a fixed class): proofs 3 and 4 of a program equal the CPU oracle's
    byte for byte with zk_prover_coeff_sources reporting the columns, under both schedules, for the push/add program
    (sparse columns below 22: BASE and ZERO columns side by side) and over the quadratic extension; the same bytes in a
    child process with ZK_COEFF_SRC=0 (no column reported); an edited fixed column is refuted and redone all-PLAIN;
  - the three consumers directly (zk_diag_coeff_sources) on random planes with a table of BASE and ZERO columns against
    the materialised planes base + w e through the all-PLAIN table: the OOD frame, the DEEP coefficients, composition
    column 0 and the degree flag agree bit for bit.  n = 64 (ood_eval's E = 1), 1024 (E = 16, one wave per column) and
    4096 (two DIV_CH = 2048 chunks, 16 DIV_T blocks); scalars 0, 1, p - 1 and random; both challenge fields; every
    column derived, and none.  Where two columns stay PLAIN their constant coefficients are chosen so that both
    assertion remainders vanish: the degree flag is then 0, and a wrong e_(n-1) weight would raise it;
  - UploadPlan::coeff_src on the CPU over the hint and switch grid.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import random
import subprocess
import sys

import pytest

import back_half_ref as ref
from test_fixed_columns import FIXED, QUAD, ROOT, get_trace, oracle_proof, other_last_row
from test_gpu_back_half import elems, ref_ints, root_of_unity
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions

P = ref.P
W = 28
PLAIN, BASE, ZERO = 0, 1, 2
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- whole proofs
def cipher_seq():
    ta, pa = get_trace(13, "cipher", 41)
    tb, pb = get_trace(13, "cipher", 42)
    return [("c13a", ta, pa), ("c13a", ta, pa), ("c13b", tb, pb), ("c13b2", other_last_row(tb), pb)]


def prove_seq(g, oracle, seq, opts=ProofOptions(), quad=False):
    """The proofs of seq on g, each the oracle's; (upload_stats, coeff_sources) of each."""
    out = []
    for name, t, p in seq:
        proof, _, _, rc = g.prove(t, p, opts)
        assert rc == 0 and proof == oracle_proof(oracle, name, t, p, quad=quad), name
        out.append((g.upload_stats(), g.coeff_sources()))
    return out


def sources_of(up):
    """The columns a proof with these upload classes reads at their source: clock, fixed, hinted sparse."""
    return sorted(set(up["derived"]) | set(up["fixed"]) | set(up["sparse"]))


@gpu
@pytest.mark.parametrize("schedule", ["throughput", "latency"])
def test_cipher_mix_third_and_fourth_proof(oracle, schedule):
    g = GpuProver(0, max_trace_len=1 << 13)
    g.set_upload_schedule(schedule)
    try:
        res = prove_seq(g, oracle, cipher_seq())
        assert [r[1] for r in res[:2]] == [[], []]  # no snapshot yet: every plane written
        for up, src in res[2:]:
            assert up["fixed"] == FIXED and up["derived"] == [0] and set(range(23, 28)) <= set(up["sparse"])
            assert src == sources_of(up)
        assert g.proof_info()["schedule"] == schedule and g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


@gpu
def test_push_add_base_and_zero_columns_mixed(oracle):
    """Opcode bits 1 .. 3 stay hinted sparse (ZERO) among the fixed columns (BASE), and the unused stack registers from
    column 12 + depth on are ZERO columns the boundary quotient reads."""
    t, p = get_trace(13, "pushadd", 43)
    g = GpuProver(0, max_trace_len=t.shape[1])
    try:
        res = prove_seq(g, oracle, [("p13", t, p)] * 4)
        for up, src in res[2:]:
            assert up["fixed"] == list(range(4, 12)) and set(range(1, 4)) <= set(up["sparse"])
            assert any(12 <= c < 20 for c in up["sparse"]), up
            assert src == sources_of(up)
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


@gpu
def test_quadratic_extension(oracle):
    g = GpuProver(0, max_trace_len=1 << 13)
    try:
        res = prove_seq(g, oracle, cipher_seq(), QUAD, quad=True)
        assert [r[1] for r in res[:2]] == [[], []]
        assert res[2][1] == res[3][1] == sources_of(res[3][0]) and res[3][0]["fixed"] == FIXED
    finally:
        g.close()


CHILD = r'''
import hashlib, json, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
from test_fixed_columns import QUAD, get_trace, other_last_row
from zkvm_amd.prover import GpuProver, ProofOptions
ta, pa = get_trace(13, "cipher", 41)
tb, pb = get_trace(13, "cipher", 42)
tp, pp = get_trace(13, "pushadd", 43)
cipher = [(ta, pa), (ta, pa), (tb, pb), (other_last_row(tb), pb)]
out = []
for seq, opts in ((cipher, ProofOptions()), ([(tp, pp)] * 4, ProofOptions()), (cipher, QUAD)):
    g = GpuProver(0, max_trace_len=1 << 13)
    for t, p in seq:
        proof, _, _, rc = g.prove(t, p, opts)
        out.append((rc, hashlib.sha256(proof).hexdigest(), g.upload_stats()["fixed"], g.coeff_sources()))
    g.close()
print("RESULT " + json.dumps(out), flush=True)
'''


@gpu
def test_switch_off_writes_the_planes_and_gives_the_same_bytes(oracle, tmp_path):
    """ZK_COEFF_SRC=0 (read once per process, so in a child): the fixed class is still taken, no column is read at its
    source, and every proof is the oracle's."""
    names = ["c13a", "c13a", "c13b", "c13b2"]
    cs = cipher_seq()
    tp, pp = get_trace(13, "pushadd", 43)
    want = [oracle_proof(oracle, nm, t, p) for nm, t, p in cs]
    want += [oracle_proof(oracle, "p13", tp, pp)] * 4
    want += [oracle_proof(oracle, nm, t, p, quad=True) for nm, t, p in cs]
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=str(ROOT), pkg=str(ROOT / "encrypt-zkvm_amd"), tests=str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-u", str(script)], env=dict(os.environ, ZK_COEFF_SRC="0"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert [(rc, sha) for rc, sha, _, _ in out] == [(0, hashlib.sha256(w).hexdigest()) for w in want], names
    assert all(src == [] for _, _, _, src in out)
    assert out[3][2] == FIXED and out[7][2] == list(range(4, 12)) and out[11][2] == FIXED  # the class itself stays on


@gpu
def test_edited_fixed_column_is_still_refuted(oracle):
    """A fixed column edited before the last row: the host compare voids the proof that read the snapshot's planes, the
    redo runs all-PLAIN from the caller's columns and fails the AIR, and valid traces keep proving to the oracle's."""
    t, p = get_trace(13, "cipher", 41)
    n = t.shape[1]
    bad = t.copy()
    bad[1, 0, 0] ^= 1
    want = oracle_proof(oracle, "c13a", t, p)
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(3):
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == want
        assert g.upload_stats()["fixed"] == FIXED and g.coeff_sources() == sources_of(g.upload_stats())
        redos = g.proof_info()["hint_redos"]
        _, _, _, rc = g.prove(bad, p, ProofOptions(), allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE and g.proof_info()["hint_redos"] == redos + 1
        assert g.coeff_sources() == []  # the redo
        proof, _, _, rc = g.prove(t, p, ProofOptions())
        assert rc == 0 and proof == want and g.upload_stats()["fixed"] == [] and g.coeff_sources() == []
    finally:
        g.close()


# ---------------------------------------------------------------- the consumers directly
def planes_bytes(planes):
    return b"".join(elems(pl) for pl in planes)


def run_consumers(planes, modes, w, cp, n, ext, z, zg, at, ac, cb, bnd1, c):
    """zk_diag_coeff_sources: (OOD frame, DEEP coefficients, composition column 0, degree flag) as integers."""
    assert native.device_count() > 0, "no GPU visible"
    flat = lambda vs: elems(vs) if ext == 1 else elems(itertools.chain.from_iterable(vs))  # noqa: E731
    ood = C.create_string_buffer(16 * ext * (56 + len(cp)))
    deep, col0 = C.create_string_buffer(16 * ext * n), C.create_string_buffer(16 * ext * n)
    flag = C.c_uint32(7)
    native.check(native.lib().zk_diag_coeff_sources(
        0, planes_bytes(planes), bytes(modes), elems(w), planes_bytes(cp), len(cp), n, ext, flat([z]), flat([zg]),
        flat(at), flat(ac), elems(itertools.chain.from_iterable(cb)), elems(bnd1), elems([c]), ood, deep, col0,
        C.byref(flag)), "zk_diag_coeff_sources")
    return ref_ints(ood.raw), ref_ints(deep.raw), ref_ints(col0.raw), flag.value


def horner(poly, x):
    acc = 0
    for v in reversed(poly):
        acc = (acc * x + v) % P
    return acc


# the assertions' columns in coefficient order (BndPoly::cb): step 0, then step n - 2
STEP0 = [0, 7, 8, 11] + list(range(12, 20))
STEPL = [7, 8] + list(range(12, 20))

MIX = [BASE] * 12 + [PLAIN, ZERO, PLAIN, PLAIN, ZERO, PLAIN, PLAIN, ZERO, PLAIN, PLAIN, PLAIN] + [ZERO] * 5
ALL = [BASE] * 12 + [ZERO, BASE] * 8
NONE = [PLAIN] * W
CASES = [(n, ext, "mix") for n in (64, 1024, 4096) for ext in (1, 2)]
CASES += [(1024, ext, kind) for kind in ("all", "none") for ext in (1, 2)]


@gpu
@pytest.mark.parametrize("n,ext,kind", CASES, ids=[f"n{n}-ext{e}-{k}" for n, e, k in CASES])
def test_consumers_from_sources_equal_materialised_planes(n, ext, kind):
    rnd = random.Random(7 * n + ext + len(kind))
    modes = {"mix": MIX, "all": ALL, "none": NONE}[kind]
    chal = (lambda: rnd.randrange(1, P)) if ext == 1 else (lambda: (rnd.randrange(1, P), rnd.randrange(P)))
    planes = [[rnd.randrange(P) for _ in range(n)] for _ in range(W + 1)]  # plane 28: e
    e = planes[W]
    derived = [c for c in range(W) if modes[c] != PLAIN]
    # scalars 0, 1, p - 1, random in turn over the derived columns; columns 0, 7, 8, 11 (the step 0 assertions' BASE
    # columns) get one of each
    w = [0] * W
    for i, c in enumerate(derived):
        w[c] = [0, 1, P - 1, rnd.randrange(P)][{0: 0, 7: 1, 8: 2, 11: 3}.get(c, i % 4)]
    C_ = 7 if ext == 1 else 4
    cp = [[rnd.randrange(P) for _ in range(n)] for _ in range(C_ * ext)]
    z, zg = chal(), chal()
    at, ac = [chal() for _ in range(W)], [chal() for _ in range(C_)]
    cb = [[rnd.randrange(P) for _ in range(22)] for _ in range(ext)]
    c = pow(root_of_unity(n.bit_length() - 1), n - 2, P)
    # the columns as the parent writes them: base + w e
    full = [planes[k] if modes[k] == PLAIN else
            [((b if modes[k] == BASE else 0) + w[k] * ev) % P for b, ev in zip(planes[k], e)] for k in range(W)]
    want_flag = None
    if modes[12] == PLAIN and modes[14] == PLAIN:
        # constant coefficients of columns 12 and 14 (12 alone over F) such that sum_k cb_k T_ck(1) = 0 in every plane
        r = [-sum(cb[j][i] * sum(full[k]) for i, k in enumerate(STEP0)) % P for j in range(ext)]
        if ext == 1:
            d12, d14 = r[0] * pow(cb[0][4], -1, P) % P, 0
        else:
            (a, b), (cc, d) = (cb[0][4], cb[0][6]), (cb[1][4], cb[1][6])
            det = pow((a * d - b * cc) % P, -1, P)
            d12, d14 = (r[0] * d - b * r[1]) * det % P, (a * r[1] - cc * r[0]) * det % P
        for k, dk in ((12, d12), (14, d14)):
            planes[k][0] = full[k][0] = (full[k][0] + dk) % P
        want_flag = 0
    # bnd1 = sum_k cb'_k T_c'k(c): the step n - 2 remainder vanishes too
    at_c = {k: horner(full[k], c) for k in STEPL}
    bnd1 = [sum(cb[j][12 + i] * at_c[k] for i, k in enumerate(STEPL)) % P for j in range(ext)]
    args = (cp, n, ext, z, zg, at, ac, cb, bnd1, c)
    got = run_consumers(planes, modes, w, *args)
    want = run_consumers(full + [e], NONE, [0] * W, *args)
    for name, g_, w_ in zip(("OOD frame", "DEEP coefficients", "composition column 0"), got, want):
        bad = [i for i, (x, y) in enumerate(zip(g_, w_)) if x != y]
        assert not bad, f"{name}: entries {bad[:8]} of {len(w_)} differ"
    assert got[3] == want[3] and (want_flag is None or got[3] == want_flag), (got[3], want[3], want_flag)
    # the all-PLAIN table against the reference frame: what every caller without sources gets
    frame = ref.ood_frame(full, cp, z, zg, ext)
    np_ = 56 + len(cp)
    assert (want[0] if ext == 1 else list(zip(want[0][:np_], want[0][np_:]))) == frame


# ---------------------------------------------------------------- the plan's decision (no GPU)
def coeff_src(n=1 << 13, have=True, sparse=0, nw8=0, nw32=0, clk_off=False, fixed_off=False, snap=False, snap_mask=0,
              hint_ok=True, no_virtual=False, lat=False, detect=True, switches=0x7F):
    arr = (C.c_uint32 * 13)(have, sparse, nw8, nw32, clk_off, fixed_off, snap, snap_mask, hint_ok, no_virtual, lat,
                            detect, switches)
    return native.lib().zk_diag_upload_plan_coeff_src(arr, n)


HINTS = dict(sparse=0x0F800000, nw8=0x70, nw32=0x1, snap=True, snap_mask=0xFFE)


def test_plan_takes_sources_only_with_a_snapshot_in_use():
    assert coeff_src(**HINTS) == 1
    assert coeff_src(**dict(HINTS, lat=True)) == 1
    assert coeff_src(**dict(HINTS, snap=False)) == 0  # the proof that takes the snapshot reads its own planes
    assert coeff_src(**dict(HINTS, snap_mask=0)) == 0
    assert coeff_src(**dict(HINTS, snap_mask=0x00E, sparse=0x0F80000E)) == 0  # every snapshot column hinted sparse
    assert coeff_src(**dict(HINTS, no_virtual=True)) == 0  # stage dumps read the trace polynomials
    assert coeff_src(**dict(HINTS, switches=0x3F)) == 0  # ZK_COEFF_SRC=0
    assert coeff_src(**dict(HINTS, have=False)) == 0
    assert coeff_src(**dict(HINTS, hint_ok=False)) == 0  # a voided proof, redone without hints
    assert coeff_src(**dict(HINTS, detect=False)) == 0
    assert coeff_src(**dict(HINTS, fixed_off=True)) == 0


@pytest.mark.parametrize("off", range(7), ids=["sparse", "narrow", "clock", "fixed", "fixed_fuse", "virtual", "coeff_src"])
def test_plan_over_the_switch_grid(off):
    """One switch off at a time, every combination of the inputs the decision depends on: on exactly when the plan forms
    columns from the snapshot (fixm != 0, worked out here from the rules), ZK_COEFF_SRC is on and no_virtual is not set.
    ZK_CLOCK, ZK_NARROW, ZK_FIXED_FUSE and ZK_VIRTUAL change the LDE side only."""
    sw = 0x7F & ~(1 << off)
    for have, hint_ok, snap, no_virtual, fixed_off, lat in itertools.product([False, True], repeat=6):
        fresh = have and hint_ok and bool(sw & 1)
        fixm = HINTS["snap_mask"] & ~HINTS["sparse"] if fresh and snap and (sw & 8) and not fixed_off else 0
        want = int(bool(sw & 64) and not no_virtual and fixm != 0)
        got = coeff_src(**dict(HINTS, have=have, hint_ok=hint_ok, snap=snap, no_virtual=no_virtual, fixed_off=fixed_off,
                               lat=lat, switches=sw))
        assert got == want, (off, have, hint_ok, snap, no_virtual, fixed_off, lat)
