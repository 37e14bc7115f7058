"""Helpers the plug-point tests over the challenge field share (tests/test_gpu_plug_ext.py, tests/test_plug_ext_cpu.py):
element arrays, the layout permutation in two independent forms, and a host model of the layout kernel's LDS image.

The references of those tests rest on one fact.  The trace and the constraints are base-field, so E enters every plug
point linearly, component by component: (a, b) c = (a c, b c) for c in F.  The a-plane of an E result is the base-field
result for the a-components of the inputs, and likewise for b; the extension's modulus never enters.
"""
import numpy as np

from zkvm_amd import plug

P = 2**128 - 45 * 2**40 + 1


def to_arr(values):
    """integers -> (len, 2) uint64 (low, high halves)"""
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little") for v in values), dtype=np.uint64).reshape(-1, 2).copy()


def to_ints(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


def rand_elems(rng, *shape):
    """uniform over the values below 2^128 - 2^64 (every one canonical: p's high half is 2^64 - 1)"""
    a = rng.integers(0, 2**64, size=(*shape, 2), dtype=np.uint64)
    a[..., 1] = rng.integers(0, 2**64 - 1, size=shape, dtype=np.uint64)
    return a


def natural_from_planes(planes, n, ext):
    """(ext, 8n, 2) coset-major planes -> (8n, 2) or (8n, 2, 2) in winterfell's order, by plug.ce_natural_order"""
    flat = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, 2)
    nat = flat[plug.ce_natural_order(n, ext)]
    return nat.reshape(8 * n, 2) if ext == 1 else nat.reshape(8 * n, 2, 2)


def planes_from_natural(nat, n, ext):
    flat = np.ascontiguousarray(nat, dtype=np.uint64).reshape(-1, 2)
    out = np.empty_like(flat)
    out[plug.ce_natural_order(n, ext)] = flat
    return out.reshape(ext, 8 * n, 2)


def natural_scalar(planes, n, ext):
    """The same by the scalar loop of prover.hip's coset_major_rows_to_host (B = 8, one column):
    o[i] = h[(i % B) * n + i / B], run per component plane, the components interleaved per element."""
    B = 8
    out = []
    for i in range(B * n):
        for k in range(ext):
            out.append(planes[k][(i % B) * n + i // B])
    return out


# ---------------------------------------------------------------- the layout kernel's LDS image (kernels.hip ce_lds)
# lane groups that share one LDS cycle (16-byte accesses): reads in four groups of 16, stores in eight groups of 8
READ_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
READ_GROUPS += [[lane + 32 for lane in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(8 * i, 8 * i + 8)) for i in range(8)]
TILE_Q = 64


def lds_index(q, c, ext):
    q0, q1, q2, q3 = q & 1, (q >> 1) & 1, (q >> 2) & 1, (q >> 3) & 1
    swz = (q3 << 3) | (q0 << 2) | (q1 << 1) | q2 if ext == 1 else ((q0 ^ q3) << 3) | (q0 << 2) | (q2 << 1) | q1
    return (q * 8 * ext + c) ^ swz


def worst_conflict(ext):
    """the largest number of lanes of one group on one 16-byte slot, per side and access: {(side, access): ways}.
    A read's slot is its index mod 16 (64 banks), a store's mod 8 (32 banks)."""
    cw = 8 * ext
    worst = {}

    def note(key, slots):
        worst[key] = max(worst.get(key, 0), max(slots.count(s) for s in slots))

    for access, groups, mod in (("read", READ_GROUPS, 16), ("write", WRITE_GROUPS, 8)):
        for c in range(cw):  # plane side: lane = q, one (coset, component) row per wave
            for g in groups:
                note(("planes", access), [lds_index(lane, c, ext) % mod for lane in g])
        for base in range(0, TILE_Q * cw, 64):  # natural side: lane = consecutive flat index
            for g in groups:
                note(("natural", access), [lds_index((base + lane) // cw, (base + lane) % cw, ext) % mod for lane in g])
    return worst
