"""The two pure rules of csrc/shard_agree.hpp, without a GPU: what the ranks of a sharded proof agree on from their
control records, and how the row windows of a sharded trace validation merge (both through the test entry points
bound in zkvm_amd/shard_diag.py) -- the merged report against tests/validate_ref.py's report of the whole trace, the
partials built from the same reference restricted to each rank's window.  Integers, bytes and strings: all exact.
"""
import ctypes as C

import pytest

from test_validate_cpu import valid_trace_128
from validate_ref import U64_MAX, ZK_ERR_TRACE, ZK_OK, add_to_cell, reference_message, reference_rc, reference_report
from zkvm_amd import native, shard_diag

WORLDS = (2, 8)
OPT = (32, 8, 0, 1, 8, 127)
HINTS = {"hint_fresh": 1, "hint_S": 0x0FF00000, "hint_clk": 1, "hint_N8": 0x3E, "hint_N32": 0x1000}
# the fields that must match, in layout order: (the record's field or (field, index), a differing value, the name)
MUST_MATCH = [("n", 256, "n")] + [(("opt", k), OPT[k] + 1, f"options.{m}") for k, m in enumerate(
    ("num_queries", "blowup", "grinding", "field_extension", "fri_folding", "fri_rem_max_deg"))] + [
    (("pub_hash", 31), 7, "public inputs"), ("source", native.SRC_DEVICE, "trace source"),
    ("split_rep", 3, "comm.trace_split"), ("measure", 1, "comm.measure")]


def records(world, **over):
    """Equal records of `world` ranks that pass every check."""
    R = (native.AgreeRecord * world)()
    for r in range(world):
        x = R[r]
        x.version, x.world, x.rank, x.status, x.n = native.AGREE_VERSION, world, r, ZK_OK, 128
        x.opt[:] = OPT
        x.pub_hash[:] = bytes(range(32))
        x.source, x.split_rep, x.measure, x.validate, x.detect = native.SRC_HOST, -1, 0, 0, 3
        for k, v in over.items():
            setattr(x, k, v)
    return R


def put(rec, field, value):
    if isinstance(field, tuple):
        getattr(rec, field[0])[field[1]] = value
    else:
        setattr(rec, field, value)


def agree(R):
    rc, d, msg = shard_diag.agree(R)
    assert rc == d["code"]
    return d, msg


def test_new_symbols_and_layout():
    L = native.lib()
    assert len(shard_diag.SYMBOLS) == 4
    for name in ("zk_comm_agreement",) + shard_diag.SYMBOLS:
        assert hasattr(L, name), name
    assert "zk_comm_agreement" in native.EXPORTED and native.ZK_ERR_PEER == -5
    assert C.sizeof(native.AgreeRecord) == 256 and C.sizeof(native.ValPartial) == 1160
    assert native.AgreeRecord.n.offset == 16 and native.AgreeRecord.pub_hash.offset == 48
    assert native.AgreeRecord.source.offset == 80 and native.AgreeRecord.msg.offset == 120


@pytest.mark.parametrize("world", WORLDS)
def test_equal_records_decide_by_and_equal_or(world):
    d, msg = agree(records(world, **HINTS))
    assert d["code"] == ZK_OK and msg == "" and (d["rank_a"], d["rank_b"]) == (-1, -1) and d["world"] == world
    assert (d["detect"], d["clock"], d["hints"], d["hints_equal"], d["validate"]) == (1, 1, 1, 1, 0)
    # equal sets that are not fresh: nothing to use, and no disagreement
    d, _ = agree(records(world))
    assert (d["hints"], d["hints_equal"]) == (0, 1)
    # detect and clock: AND, each on its own; validate: OR
    for rank in (0, world - 1):
        R = records(world, **HINTS)
        R[rank].detect = 2
        d, _ = agree(R)
        assert d["code"] == ZK_OK and (d["detect"], d["clock"]) == (0, 1)
        R[rank].detect = 1
        d, _ = agree(R)
        assert (d["detect"], d["clock"]) == (1, 0)
        R = records(world)
        R[rank].validate = 1
        d, _ = agree(R)
        assert d["code"] == ZK_OK and d["validate"] == 1


@pytest.mark.parametrize("world", WORLDS)
def test_a_refusing_rank_is_named_and_the_lowest_of_two(world):
    R = records(world)
    R[world - 1].status = native.ZK_ERR_INVALID_ARG
    R[world - 1].msg = b"trace length 128 exceeds the prover's max_trace_len 64"
    d, msg = agree(R)
    assert d["code"] == native.ZK_ERR_PEER and d["rank_a"] == world - 1 and d["field"] == "status"
    assert msg == f"rank {world - 1} refused the proof: -1: trace length 128 exceeds the prover's max_trace_len 64"
    R[1].status = native.ZK_ERR_OUT_OF_MEMORY
    R[1].msg = b"HIP error: out of memory"
    R[1].n = 64  # (a refusal comes before any comparison of fields)
    d, msg = agree(R)
    assert d["code"] == native.ZK_ERR_PEER and d["rank_a"] == 1
    assert msg == "rank 1 refused the proof: -4: HIP error: out of memory"
    # a message that fills all 120 bytes (no terminator in the record) is taken whole
    R = records(world)
    R[0].status, R[0].msg = -3, b"x" * native.AGREE_MSG
    d, msg = agree(R)
    assert d["rank_a"] == 0 and msg == "rank 0 refused the proof: -3: " + "x" * native.AGREE_MSG


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("field,value,name", MUST_MATCH, ids=[m[2] for m in MUST_MATCH])
def test_each_must_match_field_is_named(world, field, value, name):
    R = records(world)
    put(R[world - 1], field, value)
    d, msg = agree(R)
    assert d["code"] == native.ZK_ERR_INVALID_ARG and (d["rank_a"], d["rank_b"]) == (0, world - 1)
    assert msg.startswith(f"sharded proof: ranks disagree on {name}") and d["field"].startswith(name)
    assert f"(rank 0: " in msg and f", rank {world - 1}: " in msg
    # the two lowest ranks that hold different values: another differing rank above does not change them
    if world > 2:
        put(R[1], field, value)
        d, _ = agree(R)
        assert (d["rank_a"], d["rank_b"]) == (0, 1)


@pytest.mark.parametrize("world", WORLDS)
def test_the_first_differing_field_in_layout_order_is_named(world):
    for i in range(len(MUST_MATCH) - 1):
        for j in range(i + 1, len(MUST_MATCH)):
            R = records(world)
            put(R[1], MUST_MATCH[j][0], MUST_MATCH[j][1])            # the later field on a LOWER rank
            put(R[world - 1], MUST_MATCH[i][0], MUST_MATCH[i][1])    # the earlier one on the last
            d, msg = agree(R)
            assert d["code"] == native.ZK_ERR_INVALID_ARG and d["field"].startswith(MUST_MATCH[i][2]), (i, j, msg)
    R = records(world)
    R[1].world = 4 if world != 4 else 2
    R[1].n = 64
    d, msg = agree(R)
    assert d["field"] == "world" and "rank 1: 4" in msg
    R = records(world)
    R[world - 1].opt[0] = 31
    assert agree(R)[1] == f"sharded proof: ranks disagree on options.num_queries (rank 0: 32, rank {world - 1}: 31)"


@pytest.mark.parametrize("world", WORLDS)
def test_hint_sets_that_differ_give_no_hints_and_no_error(world):
    R = records(world, **HINTS)
    R[world - 1].hint_N32 ^= 1 << 9
    d, msg = agree(R)
    assert d["code"] == ZK_OK and msg == "" and (d["hints"], d["hints_equal"]) == (0, 0)
    assert (d["detect"], d["clock"]) == (1, 1)
    # a rank whose prover is new holds no set at all
    R = records(world, **HINTS)
    for k in HINTS:
        setattr(R[0], k, 0)
    d, _ = agree(R)
    assert d["code"] == ZK_OK and (d["hints"], d["hints_equal"]) == (0, 0)


@pytest.mark.parametrize("world", WORLDS)
def test_a_wrong_layout_version_is_refused(world):
    R = records(world)
    R[world - 1].version = native.AGREE_VERSION + 1
    R[0].status = -3  # (a record that cannot be read is refused before anything in it is)
    d, msg = agree(R)
    assert d["code"] == native.ZK_ERR_INVALID_ARG and d["rank_a"] == world - 1 and d["field"] == "version"
    assert f"rank {world - 1} sent a control record of layout version 2" in msg
    assert shard_diag.agree(R, world=0)[0] == native.ZK_ERR_INVALID_ARG
    assert shard_diag.agree(R, world=9)[0] == native.ZK_ERR_INVALID_ARG


# ---------------------------------------------------------------- the row split and the merge
def window(n, g, G):
    return shard_diag.val_window(n, g, G)


@pytest.mark.parametrize("n", [64, 128, 4096])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_windows_tile_the_steps_and_the_assertions(n, G):
    nxt, seen = 0, 0
    for g in range(G):
        first, count, amask = window(n, g, G)
        assert first == nxt and first == g * n // G and count >= 1
        assert amask & native.ASSERT_ROW0 == (native.ASSERT_ROW0 if first == 0 else 0)
        assert amask & native.ASSERT_LAST == (native.ASSERT_LAST if first + count == n - 2 else 0)
        assert not (seen & amask)
        seen |= amask
        nxt = first + count
    assert nxt == n - 2 and seen == (1 << 22) - 1
    # assertion k is at row 0 for k = 0, 1 and the even k, at row n - 2 for the odd k >= 3 (get_assertions' order)
    assert native.ASSERT_ROW0 == sum(1 << k for k in range(22) if k < 2 or k % 2 == 0)


def partial_of(oracle, trace, pub, g, G):
    """Rank g's partial, from the reference validator restricted to its window."""
    n = trace.shape[1]
    first, count, amask = window(n, g, G)
    rep = reference_report(oracle, trace, pub, steps=range(first, first + count))
    p = native.ValPartial()
    p.version, p.rank, p.status, p.amask, p.first, p.count = native.AGREE_VERSION, g, ZK_OK, amask, first, count
    p.failing_steps, p.a_mask = rep["failing_steps"], rep["a_mask"] & amask
    for k in range(20):
        p.t_count[k], p.t_first[k] = rep["t_count"][k], rep["t_first"][k]
        p.t_value[16 * k:16 * k + 16] = rep["t_value"][k].to_bytes(16, "little")
    for k in range(22):  # the cells this rank did not check stay as the host wrote them: the expected value
        v = rep["a_found"][k] if (amask >> k) & 1 else rep["a_expected"][k]
        p.a_found[16 * k:16 * k + 16] = v.to_bytes(16, "little")
    return p


def merge(parts, n, pub):
    return shard_diag.merge_validation(parts, n, pub)


def check_merge(oracle, trace, pub, G):
    n = trace.shape[1]
    want = reference_report(oracle, trace, pub)
    rc, got, msg = merge([partial_of(oracle, trace, pub, g, G) for g in range(G)], n, pub)
    assert got == want
    assert rc == reference_rc(want)
    if rc != ZK_OK:
        assert msg == reference_message(want)
    return got


@pytest.fixture(scope="module")
def valid():
    return valid_trace_128()


@pytest.mark.parametrize("G", [2, 4, 8])
def test_merge_of_a_valid_trace(oracle, valid, G):
    rep = check_merge(oracle, valid[0], valid[1], G)
    assert rep["first_kind"] == 0


@pytest.mark.parametrize("G", [2, 8])
def test_merge_of_disjoint_windows_with_failures_in_several(oracle, valid, G):
    trace, pub = valid
    n = trace.shape[1]
    t = trace
    for col, row in ((0, 5), (13, n // 2 - 1), (13, n // 2), (7, n - 20), (11, n - 3)):
        t = add_to_cell(t, col, row, 1)
    rep = check_merge(oracle, t, pub, G)
    assert rep["first_kind"] == 2 and rep["failing_steps"] >= 4 and rep["a_mask"] == 0


def test_merge_takes_the_lowest_first_step_and_adds_the_counts(oracle, valid):
    trace, pub = valid
    n, G = trace.shape[1], 8
    # the clock constraint (0) fails at two steps of rank 1's window and at six of rank 3's
    t = add_to_cell(trace, 0, 20, 1)
    for row in (50, 53, 56):
        t = add_to_cell(t, 0, row, 1)
    rep = check_merge(oracle, t, pub, G)
    assert rep["t_count"][0] == 8 and rep["t_first"][0] == 19
    # the rule alone, on partials in an order no row split produces: the constraint fails first in rank 3 (one step)
    # and more often, later, in rank 1 -- the merged first step and its value are rank 3's, the count the sum
    parts = [partial_of(oracle, trace, pub, g, G) for g in range(G)]
    parts[3].t_count[2], parts[3].t_first[2], parts[3].failing_steps = 1, 7, 1
    parts[3].t_value[32:48] = (1234).to_bytes(16, "little")
    parts[1].t_count[2], parts[1].t_first[2], parts[1].failing_steps = 5, 9, 5
    parts[1].t_value[32:48] = (99).to_bytes(16, "little")
    rc, got, msg = merge(parts, n, pub)
    assert rc == ZK_ERR_TRACE and got["t_count"][2] == 6 and got["t_first"][2] == 7 and got["t_value"][2] == 1234
    assert got["failing_steps"] == 6 and (got["first_kind"], got["first_index"], got["first_step"]) == (2, 2, 7)
    assert msg == "main transition constraint 2 did not evaluate to ZERO at step 7; 6 failing steps, 0 failed assertions"


@pytest.mark.parametrize("G", [2, 8])
def test_merge_of_an_assertion_failing_on_the_last_rank_only(oracle, valid, G):
    trace, pub = valid
    n = trace.shape[1]
    rep = check_merge(oracle, add_to_cell(trace, 12, n - 2, 1), pub, G)
    assert rep["first_kind"] == 1 and rep["a_mask"] == 1 << 7 and rep["first_step"] == n - 2
    # a rank reports only the assertions it checked: a set bit outside its mask is not merged
    parts = [partial_of(oracle, trace, pub, g, G) for g in range(G)]
    parts[0].a_mask = 1 << 7
    rc, got, _ = merge(parts, n, pub)
    assert rc == ZK_OK and got["a_mask"] == 0


def test_merge_names_a_rank_that_could_not_validate(oracle, valid):
    trace, pub = valid
    parts = [partial_of(oracle, trace, pub, g, 4) for g in range(4)]
    parts[2].status, parts[2].msg = native.ZK_ERR_DEVICE, b"HIP error: invalid argument"
    parts[3].status = native.ZK_ERR_DEVICE
    rc, _, msg = merge(parts, trace.shape[1], pub)
    assert rc == native.ZK_ERR_PEER and msg == "rank 2 could not validate its rows: -3: HIP error: invalid argument"
    assert U64_MAX == 2**64 - 1
