"""The plug points over the challenge field, as far as no GPU is needed: the three new entry points are declared, exported
and bound with the argument counts of their prototypes; each refuses a NULL handle before it touches a device; the numpy
permutation that tests/test_gpu_plug_ext.py uses as the layout reference is the scalar formula of the existing host
conversion; and the layout kernel's LDS image (a host copy of its index function) is a bijection on a tile that no lane
group of either side conflicts on."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import plug_ext_ref as R
from zkvm_amd import native, plug

ROOT = Path(__file__).resolve().parent.parent
NEW = ("zk_lde_new_columns", "zk_eval_constraints_ext", "zk_commit_composition_ext")


def prototype_args(name):
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/zkvm_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,count", list(zip(NEW, (7, 6, 7))))
def test_declared_exported_and_bound(name, count):
    L = native.lib()
    assert name in native.EXPORTED
    assert hasattr(L, name), f"{name} is not exported"
    args = prototype_args(name)
    assert len(args) == count, args
    assert len(getattr(L, name).argtypes) == count


def test_header_cites_the_reference_and_states_the_conventions():
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    block = text[text.index("the three plug points over the challenge field"):text.index("one proof sharded over")]
    for needle in ("prover/src/lib.rs:55-62", "prover/src/lib.rs:65-72", "build_constraint_commitment",
                   "TracePolyTable", "32 bytes", "ZK_ERR_INVALID_ARG", "ZK_ERR_DEGREE", "ends the validity"):
        assert needle in block, needle


def last_error():
    return (native.lib().zk_last_error() or b"").decode()


def test_null_handles_are_refused_without_a_device():
    L = native.lib()
    h, root = C.c_void_p(), C.create_string_buffer(32)
    cols = (C.c_void_p * 28)(*([C.c_void_p(1)] * 28))
    assert L.zk_lde_new_columns(None, cols, 16, 8, C.byref(h), root, None) == native.ZK_ERR_INVALID_ARG
    assert last_error()
    buf = C.create_string_buffer(32 * 22)
    pub = native.PubInputs()
    pub.lwe_size = 5
    for ext in (1, 2, 3):
        assert L.zk_eval_constraints_ext(None, C.byref(pub), ext, buf, buf, None) == native.ZK_ERR_INVALID_ARG
        assert last_error()
        assert L.zk_commit_composition_ext(None, None, ext, 8, C.byref(h), root, None) == native.ZK_ERR_INVALID_ARG
        assert last_error()
    assert not h


def test_the_direct_layout_call_is_exported_and_checks_its_arguments():
    """n = 0, ext = 3 and a grid cap beyond 2^20 are refused before any device is opened"""
    for n, ext, blocks in ((0, 1, 0), (1, 3, 0), (1, 1, (1 << 20) + 1)):
        with pytest.raises(native.ZkError) as e:
            plug.ce_layout_direct(np.zeros((8 * ext * n, 2), dtype=np.uint64), n, ext, True, max_blocks=blocks)
        assert e.value.code == native.ZK_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        plug.ce_layout_direct(np.zeros((8, 2), dtype=np.uint64), 16, 1, True)  # 8 elements are not 8 n


@pytest.mark.parametrize("ext", [1, 2])
def test_numpy_permutation_is_the_scalar_formula(ext):
    n = 16
    planes = [[(k << 40) | (i + 1) for i in range(8 * n)] for k in range(ext)]
    want = R.natural_scalar(planes, n, ext)
    arr = np.stack([R.to_arr(pl) for pl in planes])
    nat = R.natural_from_planes(arr, n, ext)
    assert R.to_ints(nat) == want
    # element i = r + 8 q, component k at byte 32 i + 16 k (16 i for ext = 1)
    raw = nat.tobytes()
    for i in (0, 1, 7, 8, 8 * n - 1):
        for k in range(ext):
            at = 16 * ext * i + 16 * k
            assert int.from_bytes(raw[at:at + 16], "little") == planes[k][(i % 8) * n + i // 8]
    assert np.array_equal(R.planes_from_natural(nat, n, ext), arr)
    perm = plug.ce_natural_order(n, ext)
    assert sorted(perm.tolist()) == list(range(8 * ext * n))


@pytest.mark.parametrize("ext", [1, 2])
def test_lds_image_is_a_bijection_without_bank_conflicts(ext):
    cw = 8 * ext
    assert sorted(R.lds_index(q, c, ext) for q in range(R.TILE_Q) for c in range(cw)) == list(range(R.TILE_Q * cw))
    assert R.worst_conflict(ext) == {(side, access): 1 for side in ("planes", "natural") for access in ("read", "write")}
    # the linear image, for contrast: the plane side of a read puts all 16 lanes of a group on one or two slots
    linear = [[(lane * cw) % 16 for lane in g] for g in R.READ_GROUPS]
    assert max(max(s.count(x) for x in s) for s in linear) >= 8
