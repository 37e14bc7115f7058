"""The constants the constraint evaluator folds out of the Rescue round's linear half (csrc/zk_internal.hpp
air_fold_mds / air_fold_periodic, AirConsts::pv) checked with Python integers.

Constraints 12..15 are ct_r (v_r - m0_r) with m0_r = (MDS x)_r + ark_r (+ opcode, + push term).  The kernel no longer
forms m0: per proof it holds u_k = sum_r (-ct_r) MDS[r][k] and, for the 128 CE steps j = i mod 128,
pv[j] = sum_r (-ct_r) periodic[j][1 + r].  Here both come from the library's host code (zk_diag_air_fold_host: the
function the kernel's prologue runs, and the table draw_air_consts uploads) and are compared with the sums over the
reference's MDS and ARK tables (crypto/src/rescue.rs, generated into csrc/rescue_consts.hpp), the ARK columns
interpolated over the 16-cycle and evaluated at (3 w_CE^j)^(n/16) as air/src/lib.rs:201-225 defines them."""
import ctypes as C
import re
from pathlib import Path

import pytest

from zkvm_amd import native

CSRC = Path(__file__).resolve().parent.parent / "encrypt-zkvm_amd" / "csrc"
P = 2**128 - 45 * 2**40 + 1
GEN = 3  # the coset offset of every evaluation domain


def _table(text, name):
    body = text[text.index(name):]
    body = body[:body.index("};")]
    pairs = re.findall(r"\{0x([0-9a-fA-F]+)ULL,\s*0x([0-9a-fA-F]+)ULL\}", body)
    return [int(lo, 16) | (int(hi, 16) << 64) for lo, hi in pairs]


def _root_of_unity(log_n):
    """winter-math f128: TWO_ADIC_ROOT_OF_UNITY = 3^((p-1)/2^40), squared down to order 2^log_n."""
    return pow(pow(3, (P - 1) >> 40, P), 1 << (40 - log_n), P)


def _periodic_values(col16, n, w_ce):
    """The 16-cycle column col16 (values at w_16^r) at the CE points x_j = 3 w_CE^j, j < 128: the interpolant over
    <w_16> evaluated at y = x_j^(n/16)."""
    w16 = pow(w_ce, 8 * n // 16, P)
    inv16 = pow(16, P - 2, P)
    coef = [sum(col16[r] * pow(w16, (-r * k) % 16, P) for r in range(16)) * inv16 % P for k in range(16)]
    out = []
    for j in range(128):
        y = pow(GEN * pow(w_ce, j, P) % P, n // 16, P)
        out.append(sum(c * pow(y, k, P) for k, c in enumerate(coef)) % P)
    return out


def _fold_host(ct, n):
    buf = b"".join(int(v).to_bytes(16, "little") for v in ct)
    u, pv = C.create_string_buffer(64), C.create_string_buffer(128 * 16)
    f = native.lib().zk_diag_air_fold_host
    f.argtypes, f.restype = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p], None
    f(buf, n, u, pv)
    ints = lambda b: [int.from_bytes(b.raw[16 * i:16 * i + 16], "little") for i in range(len(b.raw) // 16)]
    return ints(u), ints(pv)


COEFFS = [
    [1, 0, 0, 0], [0, 0, 0, 1], [P - 1] * 4, [0] * 4,
    [0x0123456789abcdef0123456789abcdef % P, 2**127, 45 * 2**40, P - 2],
    [pow(5, 1000 + k, P) for k in range(4)],
]


@pytest.mark.parametrize("ct", COEFFS)
def test_cube_weights_against_mds(ct):
    consts = (CSRC / "rescue_consts.hpp").read_text()
    mds = _table(consts, "ZK_MDS[16][2]")
    u, _ = _fold_host(ct, 16)
    for k in range(4):
        assert u[k] == sum((P - ct[r]) * mds[4 * r + k] for r in range(4)) % P


def test_small_table_is_abs_mds():
    consts = (CSRC / "rescue_consts.hpp").read_text()
    mds = _table(consts, "ZK_MDS[16][2]")
    src = (CSRC / "zk_internal.hpp").read_text()
    body = src[src.index("constexpr uint32_t M[16] = {"):]
    m = [int(x) for x in re.findall(r"\d+", body[body.index("{"):body.index("};")])]
    assert len(m) == 16
    # a column's four 128-bit x entry products are summed in 160 bits (acc160) before the reduction
    assert all(sum(m[4 * r + k] for r in range(4)) < 2**32 for k in range(4))
    for r in range(4):
        for k in range(4):
            assert (P - m[4 * r + k] if k % 2 == 0 else m[4 * r + k]) == mds[4 * r + k]


@pytest.mark.parametrize("n", [16, 64, 256, 1024])
def test_periodic_fold_against_ark(n):
    consts = (CSRC / "rescue_consts.hpp").read_text()
    ark = _table(consts, "ZK_ARK[")
    assert len(ark) == 128
    w_ce = _root_of_unity((8 * n).bit_length() - 1)
    cols = [_periodic_values([ark[8 * r + c] for r in range(16)], n, w_ce) for c in range(4)]
    for ct in COEFFS:
        _, pv = _fold_host(ct, n)
        for j in range(128):
            assert pv[j] == sum((P - ct[r]) * cols[r][j] for r in range(4)) % P, (ct, j)
