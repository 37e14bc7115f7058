"""validate_transition_degrees for sharded proofs (zk_degrees_sharded, zk_prover_set_validate_degrees on the ranks'
provers; kernels.hip k_cross_degrees), through the loopback communicator with rank-sized provers on one GPU.

  1. The fused cross-coset step and degree scan alone (zkvm_amd.shard_diag.degrees_parts: the production pack kernel,
     fused kernel and merge on one device, split as G ranks split them) on crafted polynomials c x^i and two-term ones,
     their CE-domain values computed here with plain integers: each range's partial, the merged tops and non-zero
     bits, and, with coefficients on, every one of the 8n coefficients.
  2. The whole check against zk_degrees_device on a full prover (pinned by tests/test_gpu_degrees.py), and at n = 128
     against tests/degrees_ref.py directly: report, status, message, every rank's stored report, and the ranks' slices
     of the coefficients reassembled; host trace and uploaded trace.
  3. The two NTT regimes (n = 4096 and 8192 at world 8) against the closed forms.
  4. The switch through zk_prove_sharded and zk_vm_prove_sharded.
  5. Refusals.
Integers, bytes and strings throughout: every comparison is exact.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from degrees_ref import P, ZK_ERR_DEGREES, ZK_OK, expected, make_report, message, pushadd_zero_last_row, reference
from test_gpu_back_half import root_of_unity
from test_gpu_eval_frames import random_trace
from test_gpu_shard_validate import prove_raw
from validate_ref import ZK_ERR_TRACE, add_to_cell
from zkvm_amd import native, shard_diag
from zkvm_amd.prover import GpuProver, ProofOptions, Program, make_pub_inputs, vm_trace
from zkvm_amd.sharded import ShardedProver
from zkvm_amd.workloads import make_workload, ops_for_trace_len, push_add_program

pytestmark = pytest.mark.gpu
ZERO_QUOTIENTS = sum(1 << k for k in (4, 5, 6, 7, 9, 10))
WORLD_N = {2: 128, 4: 256, 8: 512}  # the smallest n each world accepts under the reference options


def last_error():
    return native.lib().zk_last_error().decode()


@pytest.fixture(scope="module")
def full():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=1 << 13)
    yield g
    g.close()


@pytest.fixture(scope="module")
def ranks():
    """One loopback ShardedProver per world, rank-sized provers; world 8 also serves the two NTT regimes."""
    sps = {2: ShardedProver.loopback(2, max_trace_len=128), 4: ShardedProver.loopback(4, max_trace_len=256),
           8: ShardedProver.loopback(8, max_trace_len=1 << 13)}
    yield sps
    for sp in sps.values():
        sp.close()


# ---------------------------------------------------------------- 1. the fused kernel on crafted polynomials
def ce_values(n, terms):
    """The values of sum c x^i ((i, c) in terms) over the CE domain 3 <w_8n> in coset order: value r n + q at
    3 w_8n^r w_n^q."""
    log_n = n.bit_length() - 1
    w = root_of_unity(log_n + 3)
    out = [0] * (8 * n)
    for i, c in terms:
        gi = pow(w, 8 * i, P)
        for r in range(8):
            v = c * pow(3 * pow(w, r, P), i, P) % P
            base = r * n
            for q in range(n):
                out[base + q] = (out[base + q] + v) % P
                v = v * gi % P
    return out


def crafted(n, kg, c):
    """The issue's cases as lists of (index, coefficient) terms."""
    singles = [0, kg - 1, kg, n - 1, n, n + kg - 1, 7 * n, 8 * n - 1]
    polys = [[(i, c)] for i in singles]
    polys.append([])  # the zero polynomial
    polys.append([(kg - 1, c), (7 * n, c)])         # a low range's high block beats ...
    polys.append([(n - 1 + 6 * n, c), (7 * n, c)])  # ... the last range's lower block
    return polys


def want_partial(n, kg, g, polys):
    top, nonzero = [0] * 20, 0
    for k, terms in enumerate(polys):
        mine = [i for i, _ in terms if (i % n) // kg == g]
        if mine:
            top[k], nonzero = max(mine), nonzero | 1 << k
    return top, nonzero


_QUOT = {}


def crafted_values(n, kg, c):
    """crafted(n, kg, c) and its CE-domain values, computed once per module."""
    if (n, kg, c) not in _QUOT:
        polys = crafted(n, kg, c)
        _QUOT[n, kg, c] = (polys, [ce_values(n, t) for t in polys])
    return _QUOT[n, kg, c]


PARTS = [(128, 2, 0), (128, 4, 0), (128, 8, 0), (8192, 8, 0), (8192, 8, 3)]


@pytest.mark.parametrize("n,G,max_blocks", PARTS, ids=[f"n{n}-G{G}-b{b}" for n, G, b in PARTS])
def test_fused_kernel_on_crafted_polynomials(n, G, max_blocks):
    """max_blocks = 3 at kg = 1024: four blocks' worth of k1 on a grid of three, so the launcher's stride runs a
    second, partial pass (one block of three has work in it)."""
    kg = n // G
    for c in (1, P - 1):
        polys, quot = crafted_values(n, kg, c)
        tops = [max((i for i, _ in t), default=0) for t in polys] + [0] * (20 - len(polys))
        nz = sum(1 << k for k, t in enumerate(polys) if t)
        merged_want = make_report(n, tops, ((1 << 20) - 1) & ~nz)
        for coeffs in (True, False):
            res = shard_diag.degrees_parts(quot, n, G, coeffs=coeffs, max_blocks=max_blocks)
            rc, parts, merged = res[:3]
            assert rc == ZK_ERR_DEGREES and merged == merged_want, (c, coeffs)
            for g in range(G):
                p = parts[g]
                assert (p.version, p.rank, p.status, p.first, p.count) == (native.AGREE_VERSION, g, ZK_OK, g * kg, kg)
                assert (list(p.top), p.nonzero) == want_partial(n, kg, g, polys), (c, coeffs, g)
            if coeffs:
                for k, terms in enumerate(polys):
                    want = [0] * (8 * n)
                    for i, cc in terms:
                        want[i] = cc
                    assert res[3][k] == want, f"polynomial {k}: a coefficient differs"


def test_fused_kernel_refusals():
    z = [[0] * (8 * 16)]
    for n, G in ((16, 4), (16, 3), (24, 2)):
        with pytest.raises(native.ZkError):
            shard_diag.degrees_parts([[0] * (8 * n)], n, G)
    with pytest.raises(native.ZkError):
        shard_diag.degrees_parts([[P] + z[0][1:]], 16, 2)  # a value that is not canonical


# ---------------------------------------------------------------- 2. the whole check against the single-GPU one
def crafted_pub(lwe_size):
    return make_pub_inputs([0, 0], [0] * 16, lwe_size, 16)


_VM = {}


def pushadd_source(log_n):
    """ops_for_trace_len's push/add program; at 2^7 rows, below its range, the push/add program that pads to them."""
    return push_add_program(3) if log_n == 7 else ops_for_trace_len(log_n, "pushadd")


def vm_case(log_n, last):
    """A push/add VM trace of 2^log_n rows with its public inputs; last: "random" (the workload's own) or "zero"."""
    if log_n not in _VM:
        src = pushadd_source(log_n)
        w = make_workload(src, seed=7)
        trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
        assert trace.shape[1] == 1 << log_n
        pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
        _VM[log_n] = (trace, pub, src, w)
    trace, pub, _, _ = _VM[log_n]
    if last == "zero":
        trace = trace.copy()
        trace[:, -1, :] = 0
    return trace, pub


def whole_cases(n):
    log_n = n.bit_length() - 1
    return [("random1", random_trace(n, 900 + n), crafted_pub(1)),
            ("random5", random_trace(n, 905 + n), crafted_pub(5)),
            ("vm", *vm_case(log_n, "random")), ("vm0", *vm_case(log_n, "zero"))]


def reassemble(slices, n, world):
    """The ranks' slices [k][k2][kl] -> 20 lists of 8n coefficients."""
    kg = n // world
    out = [[0] * (8 * n) for _ in range(20)]
    for g, s in enumerate(slices):
        for k in range(20):
            for k2 in range(8):
                out[k][k2 * n + g * kg:k2 * n + (g + 1) * kg] = s[k][k2]
    return out


@pytest.mark.parametrize("world", [2, 4, 8])
def test_whole_check_equals_the_single_gpu_check(oracle, full, ranks, world):
    n, sp = WORLD_N[world], ranks[world]
    for name, trace, pub in whole_cases(n):
        d, _ = full.upload_trace(trace)
        rc0, want, quot0 = full.degrees_device(d, n, pub, quotients=True)
        msg0 = last_error()
        assert rc0 == (ZK_OK if name == "vm" else ZK_ERR_DEGREES), name
        if n == 128:
            coeffs, rep, msg = reference(oracle, trace, pub.lwe_size, pub.delta)
            assert want == rep and quot0 == coeffs and (rc0 == ZK_OK or msg0 == msg)
        for source in ("host", "device"):
            if source == "host":
                rc, got, slices = sp.degrees_host(trace, pub, quotients=True)
            else:
                rc, got, slices = sp.degrees_device(sp.upload_trace(trace), pub, quotients=True)
            err = last_error()
            assert (rc, got) == (rc0, want), (name, source)
            if rc != ZK_OK:
                assert err == msg0
            assert all(sp.degrees(l) == want for l in range(world))
            assert reassemble(slices, n, world) == quot0, (name, source)
            a = sp.agreement()
            assert a["code"] == ZK_OK and a["control_calls"] == 2
            stats = sp.exchange_stats()
            assert set(stats) == {"control", "degrees_slices", "degrees_report"}
            assert stats["degrees_slices"][1:] == (20 * 8 * (n // world) * 16 * (world - 1) // world, 1)
        # without the coefficients: the kernel's other instance, the same report
        rc, got = sp.degrees_host(trace, pub)
        assert (rc, got) == (rc0, want), name


# ---------------------------------------------------------------- 3. the two NTT regimes, degrees only
@pytest.mark.parametrize("log_n", [12, 13])
def test_ntt_regimes_against_the_closed_forms(ranks, log_n):
    n, sp = 1 << log_n, ranks[8]
    trace, pub = vm_case(log_n, "random")
    rc, got = sp.degrees_device(sp.upload_trace(trace), pub)
    assert rc == ZK_OK and got == make_report(n, expected(n), 0)
    trace, pub = vm_case(log_n, "zero")
    rc, got = sp.degrees_host(trace, pub)
    want = make_report(n, pushadd_zero_last_row(n), ZERO_QUOTIENTS)
    assert rc == ZK_ERR_DEGREES and got == want and last_error() == message(want)


# ---------------------------------------------------------------- 4. the switch
def set_switches(sp, validate, degrees_rank):
    """zk_prover_set_validate on every rank; zk_prover_set_validate_degrees on rank `degrees_rank` only (None: off)."""
    L = native.lib()
    for l, p in enumerate(sp.provers):
        native.check(L.zk_prover_set_validate(p, 1 if validate else 0))
        native.check(L.zk_prover_set_validate_degrees(p, 1 if l == degrees_rank else 0))


@pytest.mark.parametrize("world", [2, 8])
def test_the_switch_through_the_sharded_proof(full, world):
    n = WORLD_N[world]
    log_n = n.bit_length() - 1
    opts = ProofOptions()
    good, pub = vm_case(log_n, "random")
    zero, _ = vm_case(log_n, "zero")
    single, _, _, rc = full.prove(good, pub, opts)
    assert rc == ZK_OK
    rc0, want0 = full.degrees_host(zero, pub)
    msg0 = last_error()
    assert rc0 == ZK_ERR_DEGREES
    sp = ShardedProver.loopback(world, max_trace_len=n)
    try:
        # switches off: both traces prove, the zero last row silently
        rc, good_off, _, msg = prove_raw(sp, good, pub, opts)
        assert rc == ZK_OK and good_off == single, msg
        rc, zero_off, _, msg = prove_raw(sp, zero, pub, opts)
        assert rc == ZK_OK and zero_off, msg
        assert sp.agreement()["validate_degrees"] == 0 and "degrees_slices" not in sp.exchange_stats()
        # both switches, one broken cell: Trace::validate comes first, and no degree check runs
        set_switches(sp, True, world - 1)
        rc, proof, plen, _ = prove_raw(sp, add_to_cell(good, 0, n // 2, 1), pub, opts)
        assert rc == ZK_ERR_TRACE and plen == 0
        assert set(sp.exchange_stats()) == {"control", "validate_report"}
        with pytest.raises(native.ZkError):
            sp.degrees()  # no degree report has been written on this prover
        # both switches, a valid trace with a zero last row: the validation passes, the degrees do not
        rc, proof, plen, msg = prove_raw(sp, zero, pub, opts)
        assert rc == ZK_ERR_DEGREES and plen == 0 and msg == msg0
        assert all(sp.validation(l)["first_kind"] == 0 for l in range(world))
        assert set(sp.exchange_stats()) == {"control", "validate_report", "degrees_slices", "degrees_report"}
        # the degree switch alone, on at the LAST rank only (OR)
        set_switches(sp, False, world - 1)
        for source in ("host", "device"):
            if source == "host":
                rc, proof, plen, msg = prove_raw(sp, zero, pub, opts)
            else:
                rc, proof, plen, msg = prove_raw(sp, None, pub, opts, n=sp.upload_trace(zero))
            assert rc == ZK_ERR_DEGREES and plen == 0 and proof == b"" and msg == msg0
            a = sp.agreement()
            assert a["validate_degrees"] == 1 and a["validate"] == 0 and a["control_calls"] == 2
            assert set(sp.exchange_stats()) == {"control", "degrees_slices", "degrees_report"}
            assert all(sp.degrees(l) == want0 for l in range(world))
        # a trace that passes goes on to the same proof bytes
        rc, proof, _, msg = prove_raw(sp, good, pub, opts)
        assert rc == ZK_OK and proof == good_off == single, msg
        stats = sp.exchange_stats()
        assert stats["degrees_slices"][2] == 1 and stats["degrees_report"][2] == 1 and stats["openings"][2] >= 1
        rc, proof, _, msg = prove_raw(sp, None, pub, opts, n=sp.upload_trace(good))
        assert rc == ZK_OK and proof == single, msg
        # afterwards, the switches off: the zero last row proves to the bytes it had before
        set_switches(sp, False, None)
        rc, proof, _, msg = prove_raw(sp, zero, pub, opts)
        assert rc == ZK_OK and proof == zero_off, msg
        assert sp.agreement()["validate_degrees"] == 0 and "degrees_slices" not in sp.exchange_stats()
    finally:
        sp.close()


@pytest.mark.parametrize("world", [2, 8])
def test_vm_prove_sharded_checks_the_written_trace(world):
    log_n = WORLD_N[world].bit_length() - 1
    vm_case(log_n, "random")
    _, _, src, w = _VM[log_n]
    prog = Program(src)
    sp = ShardedProver.loopback(world, max_trace_len=1 << log_n)
    try:
        inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
        _, _, plain = sp.prove_program(prog, inputs, w.last_row, ProofOptions())
        assert sp.agreement()["validate_degrees"] == 0
        set_switches(sp, False, world - 1)
        _, _, proof = sp.prove_program(prog, inputs, w.last_row, ProofOptions())
        a = sp.agreement()
        assert proof == plain and a["validate_degrees"] == 1 and a["control_calls"] == 2
        assert sp.degrees(0)["mismatch_mask"] == 0
        with pytest.raises(native.ZkError) as e:
            sp.prove_program(prog, inputs, [0] * 28, ProofOptions())
        assert e.value.code == ZK_ERR_DEGREES
        want = make_report(1 << log_n, pushadd_zero_last_row(1 << log_n), ZERO_QUOTIENTS)
        assert last_error() == message(want) and sp.degrees(world - 1) == want
        assert set(sp.exchange_stats()) == {"control", "degrees_slices", "degrees_report"}
        sp.set_validate_degrees(False)
        _, _, proof = sp.prove_program(prog, inputs, w.last_row, ProofOptions())
        assert proof == plain
    finally:
        sp.close()
        prog.close()


# ---------------------------------------------------------------- 5. refusals, before any launch
def degrees_raw(sp, trace, pub, n=0):
    """zk_degrees_sharded -> (rc, zk_last_error)."""
    L = native.lib()
    if trace is not None:
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        n = trace.shape[1]
    arr = (C.c_void_p * len(sp.provers))(*[p.value for p in sp.provers])
    d = native.Degrees()
    rc = L.zk_degrees_sharded(sp.comm, arr, len(sp.provers), trace.ctypes.data if trace is not None else None, n,
                              C.byref(pub), C.byref(d), None)
    return rc, L.zk_last_error().decode()


def test_refusals_are_a_sharded_proofs(ranks):
    sp, opts = ranks[8], ProofOptions()
    cases = [(np.zeros((28, 96, 2), dtype=np.uint64), crafted_pub(5)),  # no power of two
             (np.zeros((28, 64, 2), dtype=np.uint64), crafted_pub(5)),  # too short for 8 ranks
             (random_trace(512, 1), crafted_pub(0)), (random_trace(512, 1), crafted_pub(6))]
    for trace, pub in cases:
        rc0, _, _, msg0 = prove_raw(sp, trace, pub, opts)
        assert rc0 == native.ZK_ERR_INVALID_ARG
        rc, msg = degrees_raw(sp, trace, pub)
        assert (rc, msg) == (rc0, msg0) and msg
        assert set(sp.exchange_stats()) == {"control"}
        a = sp.agreement()
        assert a["code"] == native.ZK_ERR_PEER and a["field"] == "status"
    # the shortest length the 8 ranks do accept
    rc, msg = degrees_raw(sp, random_trace(128, 2), crafted_pub(5))
    assert rc == ZK_ERR_DEGREES, msg


class ThreadGroup:
    """A host-exchange transport between the threads of this process, one rank each (native.EXCHANGE_FN)."""

    def __init__(self, world):
        self.world, self.slots = world, [b""] * world
        self.bar = threading.Barrier(world, timeout=30)

    def fn(self, rank):
        def exchange(ctx, op, send, recv, nbytes):
            try:
                gather = op == native.XCHG_ALL_GATHER
                self.slots[rank] = C.string_at(send, nbytes if gather else nbytes * self.world)
                self.bar.wait()
                for s in range(self.world):
                    chunk = self.slots[s] if gather else self.slots[s][rank * nbytes:(rank + 1) * nbytes]
                    C.memmove(recv + s * nbytes, chunk, nbytes)
                self.bar.wait()
                return 0
            except Exception:  # a broken barrier: the library reports the failed callback
                return 1
        return native.EXCHANGE_FN(exchange)


def test_ranks_given_different_n_are_told_so():
    """Two ranks over a host-exchange communicator, one thread each: rank 1 is handed a trace twice as long."""
    group = ThreadGroup(2)
    sps = [ShardedProver.host(r, 2, group.fn(r), 0, 256) for r in range(2)]
    out = [None, None]
    try:
        def run(r, n):
            out[r] = degrees_raw(sps[r], random_trace(n, 3), crafted_pub(5)) + (sps[r].agreement(),)
        for lengths in ((128, 256), (128, 128)):
            ts = [threading.Thread(target=run, args=(r, lengths[r])) for r in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join(60)
            assert all(o is not None for o in out)
            if lengths[0] != lengths[1]:
                for rc, msg, a in out:
                    assert rc == native.ZK_ERR_INVALID_ARG
                    assert msg == "sharded proof: ranks disagree on n (rank 0: 128, rank 1: 256)"
                    assert a["field"] == "n" and (a["rank_a"], a["rank_b"]) == (0, 1) and a["control_calls"] == 1
            else:  # the same communicators and provers, equal inputs: the check as always, the same on both ranks
                assert out[0][:2] == out[1][:2] and out[0][0] == ZK_ERR_DEGREES
                assert sps[0].degrees() == sps[1].degrees()
            out[:] = [None, None]
    finally:
        for sp in sps:
            sp.close()


def test_a_full_prover_still_checks_on_its_own(full):
    trace, pub = vm_case(7, "random")
    d, n = full.upload_trace(trace)
    rc, got = full.degrees_device(d, n, pub)
    assert rc == ZK_OK and got == make_report(n, expected(n), 0)
    # ... and a rank-sized prover still refuses the single-GPU entry point
    sp = ShardedProver.loopback(2, max_trace_len=128)
    try:
        out = native.Degrees()
        buf = C.c_void_p()
        native.check(native.lib().zk_prover_trace_buffer(sp.provers[0], C.byref(buf)))
        rc = native.lib().zk_degrees_device(sp.provers[0], buf, 128, C.byref(pub), C.byref(out), None)
        assert rc == native.ZK_ERR_INVALID_ARG and "zk_prover_create_shard" in last_error()
    finally:
        sp.close()
