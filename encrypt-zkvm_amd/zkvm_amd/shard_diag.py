"""The test entry points of the sharded prover's agreement, row-split validation and degree check (csrc/diag.hip, the
last sections; the pure rules are csrc/shard_agree.hpp): their ctypes bindings and one Python call each.  Tests and
tools go through these calls; native.py keeps the records' layouts (AgreeRecord, ValPartial, DegPartial, Agreement).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native

# the C names, in the order of the calls below
SYMBOLS = tuple("zk_diag_" + s for s in ("agree", "val_window", "merge_validation", "validate_window"))
DEGREE_SYMBOLS = ("zk_diag_merge_degrees", "zk_diag_degrees_parts")  # the sharded degree check's two
_bound = False


def _lib():
    global _bound
    L = native.lib()
    if not _bound:
        vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
        agree_fn, window_fn, merge_fn, launch_fn = (getattr(L, s) for s in SYMBOLS)
        dmerge_fn, dparts_fn = (getattr(L, s) for s in DEGREE_SYMBOLS)
        # (records[world x 256], world, out, msg, cap)
        agree_fn.argtypes = [vp, i32, C.POINTER(native.Agreement), C.c_char_p, sz]
        # (n, g, G, out[3] = first, count, assertion mask)
        window_fn.argtypes = [C.c_uint64, i32, i32, C.POINTER(C.c_uint64)]
        # (partials[world x 1160], world, n, pub, out)
        merge_fn.argtypes = [vp, i32, sz, C.POINTER(native.PubInputs), C.POINTER(native.Validation)]
        # (device, trace, n, first, count, amask, pub, packed, partial_out)
        launch_fn.argtypes = [i32, vp, sz, sz, sz, u32, C.POINTER(native.PubInputs), i32, vp]
        # (partials[world x 312], world, n, out)
        dmerge_fn.argtypes = [vp, i32, sz, C.POINTER(native.Degrees)]
        # (device, quot[count 8n], n, count, G, max_blocks, partials_out[G x 312], merged_out, coeffs_out[count 8n])
        dparts_fn.argtypes = [i32, vp, sz, i32, i32, u32, vp, C.POINTER(native.Degrees), vp]
        _bound = True
    return L


def agree(records, world: int | None = None):
    """The agreement rule on a ctypes array of native.AgreeRecord -> (status, outcome dict, message)."""
    a = native.Agreement()
    msg = C.create_string_buffer(512)
    rc = getattr(_lib(), SYMBOLS[0])(C.addressof(records), len(records) if world is None else world, C.byref(a), msg,
                                     len(msg))
    return rc, a.to_dict(), msg.value.decode()


def val_window(n: int, g: int, G: int):
    """Rank g of G's window of a trace of n rows -> (first step, count, assertion mask)."""
    out = (C.c_uint64 * 3)()
    native.check(getattr(_lib(), SYMBOLS[1])(n, g, G, out), SYMBOLS[1])
    return out[0], out[1], out[2]


def merge_validation(parts, n: int, pub):
    """The merge of a list of native.ValPartial -> (status, report dict, zk_last_error text)."""
    arr = (native.ValPartial * len(parts))(*parts)
    v = native.Validation()
    L = _lib()
    rc = getattr(L, SYMBOLS[2])(C.addressof(arr), len(parts), n, C.byref(pub), C.byref(v))
    return rc, v.to_dict(), L.zk_last_error().decode()


def validate_window(trace, pub, first: int, count: int, amask: int, packed: int, device: int = 0):
    """One window launch of the validator on a (28, n, 2) uint64 host trace -> (status, native.ValPartial).
    packed = 0: the whole trace goes up and the window is read in place; 1: only the window's rows go up."""
    t = np.ascontiguousarray(trace, dtype=np.uint64)
    p = native.ValPartial()
    rc = getattr(_lib(), SYMBOLS[3])(device, t.ctypes.data, t.shape[1], first, count, amask, C.byref(pub), packed,
                                     C.addressof(p))
    return rc, p


def merge_degrees(parts, n: int):
    """The merge of a list of native.DegPartial -> (status, report dict, zk_last_error text)."""
    arr = (native.DegPartial * len(parts))(*parts)
    d = native.Degrees()
    L = _lib()
    rc = getattr(L, DEGREE_SYMBOLS[0])(C.addressof(arr), len(parts), n, C.byref(d))
    return rc, d.to_dict(), L.zk_last_error().decode()


def degrees_parts(quot, n: int, G: int, coeffs: bool = False, max_blocks: int = 0, device: int = 0):
    """Steps 3 to 6 of a sharded degree check on quotient values of the caller's choice, split into G ranges on one
    device.  quot: `count` lists of 8n ints, the values of each polynomial over the CE domain in coset order
    (value r n + q at 3 w_8n^r w_n^q).  -> (status, [native.DegPartial] * G, merged report dict[, coefficients: count
    lists of 8n ints])."""
    from .prover import bytes_elems, elems_bytes
    count = len(quot)
    flat = np.frombuffer(elems_bytes([v for plane in quot for v in plane]), dtype=np.uint8)
    parts = (native.DegPartial * G)()
    d = native.Degrees()
    out = np.zeros(count * 8 * n * 16, dtype=np.uint8) if coeffs else None
    rc = getattr(_lib(), DEGREE_SYMBOLS[1])(device, flat.ctypes.data, n, count, G, max_blocks, C.addressof(parts),
                                            C.byref(d), out.ctypes.data if coeffs else None)
    if rc not in (native.ZK_OK, native.ZK_ERR_DEGREES):
        native.check(rc, DEGREE_SYMBOLS[1])
    if not coeffs:
        return rc, list(parts), d.to_dict()
    c = bytes_elems(out.tobytes())
    return rc, list(parts), d.to_dict(), [c[k * 8 * n:(k + 1) * 8 * n] for k in range(count)]
