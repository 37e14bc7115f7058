"""The W sets the host builds for the constraint evaluator's launch-uniform multipliers (csrc/kernels.hip
air_build_ws, AirConsts::ws, indices EvalWs in csrc/zk_internal.hpp) checked with Python integers.

The kernel multiplies by the composition coefficients, their folds and delta through W sets: for a constant w the four
values w 2^(32 i) mod p, i < 4, stored as word 4 j + i = 32-bit word j of W_i.  zk_diag_air_ws_host runs the function
draw_air_consts runs (through set_coeff_derived) on given coefficients; every word of every set is compared with the
integer definition of its constant:
  EW_CT + k   coeff_t[k], but coeff_t[k] 3^-72 for k = 12..15     EW_NCT + r   -coeff_t[12 + r], r < 2
  EW_U + k    sum_r (-coeff_t[12 + r]) MDS[r][k]                  EW_D89       coeff_t[9] - coeff_t[8]
  EW_DELTA    delta                                               EW_CB + k    coeff_b[k]
Coefficient vectors carry the edge values 0, 1, p - 1 and values with a zero top word in every position."""
import ctypes as C
import random
import re
from pathlib import Path

import pytest

from zkvm_amd import native

CSRC = Path(__file__).resolve().parent.parent / "encrypt-zkvm_amd" / "csrc"
P = 2**128 - 45 * 2**40 + 1
EW_CT, EW_NCT, EW_U, EW_D89, EW_DELTA, EW_CB, EW_COUNT = 0, 20, 22, 26, 27, 28, 50
EDGES = [0, 1, P - 1, 2**96 - 1, 2**96, 2**32 - 1, 2**64, P - 2, 45 * 2**40, 2**127]


def _mds():
    text = (CSRC / "rescue_consts.hpp").read_text()
    body = text[text.index("ZK_MDS[16][2]"):]
    body = body[:body.index("};")]
    pairs = re.findall(r"\{0x([0-9a-fA-F]+)ULL,\s*0x([0-9a-fA-F]+)ULL\}", body)
    return [int(lo, 16) | (int(hi, 16) << 64) for lo, hi in pairs]


def _ws_host(ct, cb, delta):
    b = lambda vals: b"".join(int(v).to_bytes(16, "little") for v in vals)
    out = C.create_string_buffer(64 * EW_COUNT)
    f = native.lib().zk_diag_air_ws_host
    f.argtypes, f.restype = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p], None
    f(b(ct), b(cb), b([delta]), out)
    words = [int.from_bytes(out.raw[4 * i:4 * i + 4], "little") for i in range(16 * EW_COUNT)]
    return [words[16 * s:16 * s + 16] for s in range(EW_COUNT)]


def _ws_int(w):
    """make_fe_ws with integers: word 4 j + i = 32-bit word j of w 2^(32 i) mod p."""
    out = [0] * 16
    for i in range(4):
        v = w * 2**(32 * i) % P
        for j in range(4):
            out[4 * j + i] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def _expected(ct, cb, delta):
    mds = _mds()
    inv3_72 = pow(pow(3, 72, P), P - 2, P)
    want = [None] * EW_COUNT
    for k in range(20):
        want[EW_CT + k] = ct[k] * inv3_72 % P if 12 <= k < 16 else ct[k]
    for r in range(2):
        want[EW_NCT + r] = (P - ct[12 + r]) % P
    for k in range(4):
        want[EW_U + k] = sum((P - ct[12 + r]) * mds[4 * r + k] for r in range(4)) % P
    want[EW_D89] = (ct[9] - ct[8]) % P
    want[EW_DELTA] = delta
    for k in range(22):
        want[EW_CB + k] = cb[k]
    assert all(v is not None and 0 <= v < P for v in want)
    return want


def _cases():
    rnd = random.Random(20)
    cases = []
    for shift in range(len(EDGES)):  # every edge value in every position
        ct = [EDGES[(k + shift) % len(EDGES)] for k in range(20)]
        cb = [EDGES[(2 * k + shift) % len(EDGES)] for k in range(22)]
        cases.append((ct, cb, EDGES[shift]))
    for v in (0, 1, P - 1):
        cases.append(([v] * 20, [v] * 22, v))
    for _ in range(4):
        cases.append(([rnd.randrange(P) for _ in range(20)], [rnd.randrange(P) for _ in range(22)], rnd.randrange(2**64)))
    return cases


@pytest.mark.parametrize("case", range(len(_cases())))
def test_every_w_set_against_integers(case):
    ct, cb, delta = _cases()[case]
    got = _ws_host(ct, cb, delta)
    for s, w in enumerate(_expected(ct, cb, delta)):
        assert got[s] == _ws_int(w), f"W set {s} of the constant {w:#x}"

