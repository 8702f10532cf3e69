"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the policy observation
(tests/emul/jxs_emul_env_observe.cpp), which runs ``jxs_obs::slot_value`` of jaxsim_amd/csrc/jxs_env_observe.h over every
word of the tensor.

The library is the one of tests/env_emul_lib.py.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
declare(("jxs_emul_observe_table_error", _i, [_vp, _ll, _i, _vp, C.POINTER(_i)]),
        ("jxs_emul_observe_affine_ok", _i, [C.c_double, _i]),
        ("jxs_emul_observe_derived_used", C.c_uint, [_vp, _i, _i]),
        ("jxs_emul_env_observe", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _ll, _i, _i]))  # fmt: skip


def _slots(slots) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1, 3))


def _rows4(source_rows) -> np.ndarray:
    r = np.zeros(4, np.int32)
    if source_rows is not None:
        r[: len(source_rows)] = source_rows
    return r


def table_error(slots, n_rows: int, source_rows=None, D=None) -> tuple[int, int]:
    """``(error code of jxs_obs::table_error, slot it is in)``; ``D`` overrides the number of slots handed over."""
    s = _slots(slots)
    bad = C.c_int(-1)
    code = lib().jxs_emul_observe_table_error(_ptr(s) if s.size else None, len(s) if D is None else D, n_rows, _ptr(_rows4(source_rows)), C.byref(bad))
    return code, bad.value


def affine_ok(v: float, dtype) -> bool:
    return bool(lib().jxs_emul_observe_affine_ok(float(v), np.dtype(dtype).itemsize))


def derived_used(slots, repr_: int) -> int:
    s = _slots(slots)
    return int(lib().jxs_emul_observe_derived_used(_ptr(s), len(s), repr_))


def observe(storage: np.ndarray, slots, offset, scale, n_rows: int, n_joints: int, N: int, T: int, repr_: int, *, sources=(), out=None,
            out_ld=None, out_dtype=None, rc=False):  # fmt: skip
    """The tensor ``[N, out_ld]`` of the harness.  ``storage``: the tiled state block (flat); ``sources``: up to four tiled
    blocks as ``(flat storage, rows)`` or ``None``; ``out``: a flat array to write into (copied first).  ``rc=True``: the return code."""
    s = _slots(slots)
    D = len(s)
    dt = storage.dtype
    off = np.ascontiguousarray(np.broadcast_to(np.asarray(offset, dtype=dt), (D,)))
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=dt), (D,)))
    ld = D if out_ld is None else int(out_ld)
    odt = np.dtype(out_dtype or dt)
    res = np.zeros(N * ld, odt) if out is None else np.ascontiguousarray(out).copy()
    assert res.dtype == odt and res.size >= N * ld
    keep = [None if x is None else np.ascontiguousarray(x[0], dtype=dt) for x in sources] + [None] * (4 - len(sources))
    ptrs = (C.c_void_p * 4)(*[None if k is None else k.ctypes.data for k in keep])
    rows = _rows4([0 if x is None else x[1] for x in sources])
    code = lib().jxs_emul_env_observe(_ptr(np.ascontiguousarray(storage)), ptrs, _ptr(rows), _ptr(s), _ptr(off), _ptr(sc), D, n_rows, n_joints, int(repr_),
                                      N, T, _ptr(res), ld, dt.itemsize, odt.itemsize)  # fmt: skip
    if rc:
        return code
    assert code == 0, code
    return res if out is not None else res.reshape(N, ld)
