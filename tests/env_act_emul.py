"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the action-to-torque law
(tests/emul/jxs_emul_env_act.cpp), which runs ``jxs_act::torque_word`` of jaxsim_amd/csrc/jxs_env_act.h over every word of
the tiled torque block.

The library is the one of tests/env_emul_lib.py.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i, _ll, _d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
declare(("jxs_emul_act_table_error", _i, [_vp, _vp, _ll, _ll, _i, C.POINTER(_i)]),
        ("jxs_emul_act_finite_ok", _i, [_d, _i]), ("jxs_emul_act_limit_ok", _i, [_d, _i]),
        ("jxs_emul_act_targets_ok", _i, [_d, _d, _i]), ("jxs_emul_act_pack_roundtrip", _i, [_i, _i]),
        ("jxs_emul_env_act", _i, [_vp, _vp, _ll, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i]))  # fmt: skip


def _table(joints, params):
    j = np.ascontiguousarray(np.asarray(joints, dtype=np.int32).reshape(-1, 2))
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, 8))
    assert len(j) == len(p)
    return j, p


def table_error(joints, params, A: int, dtype, n=None) -> tuple[int, int]:
    """``(error code of jxs_act::table_error, joint it is in)``; ``n`` overrides the number of joints handed over."""
    j, p = _table(joints, params)
    bad = C.c_int(-7)
    code = lib().jxs_emul_act_table_error(_ptr(j) if j.size else None, _ptr(p) if p.size else None, len(j) if n is None else n, A,
                                          np.dtype(dtype).itemsize, C.byref(bad))  # fmt: skip
    return code, bad.value


def finite_ok(v: float, dtype) -> bool:
    return bool(lib().jxs_emul_act_finite_ok(float(v), np.dtype(dtype).itemsize))


def limit_ok(v: float, dtype) -> bool:
    return bool(lib().jxs_emul_act_limit_ok(float(v), np.dtype(dtype).itemsize))


def targets_ok(lo: float, hi: float, dtype) -> bool:
    return bool(lib().jxs_emul_act_targets_ok(float(lo), float(hi), np.dtype(dtype).itemsize))


def pack_roundtrip(mode: int, column: int) -> bool:
    return lib().jxs_emul_act_pack_roundtrip(mode, column) == 0


def act(storage: np.ndarray, joints, params, actions, n_rows: int, N: int, T: int, *, A=None, feed_forward=None, out=None, rc=False):
    """The flat tiled torque block ``[ceil(N/T)][n][T]`` of the harness.  ``storage``: the tiled state block (flat);
    ``actions``: ``[N, act_ld]`` float32 or the state's dtype, or ``None``; ``feed_forward``: a flat tiled ``[n][N]`` block or
    ``None``; ``out``: a flat array to write into (copied first).  ``rc=True``: the return code."""
    j, p = _table(joints, params)
    n = len(j)
    dt = storage.dtype
    words = -(-N // T) * n * T
    res = np.zeros(words, dt) if out is None else np.ascontiguousarray(out).copy()
    assert res.dtype == dt and res.size >= words
    if actions is None:
        acts, ld, ab = None, 0 if A is None else A, dt.itemsize
    else:
        acts = np.ascontiguousarray(actions)
        assert acts.ndim == 2 and acts.shape[0] >= N
        ld, ab = acts.shape[1], acts.dtype.itemsize
    width = (int(j[:, 1].max()) + 1 if acts is None else ld) if A is None else int(A)
    ff = None if feed_forward is None else np.ascontiguousarray(feed_forward, dtype=dt)
    code = lib().jxs_emul_env_act(_ptr(np.ascontiguousarray(storage)), _ptr(acts), ld, width, _ptr(j), _ptr(p), n, n_rows, _ptr(ff), _ptr(res), N, T,
                                  dt.itemsize, ab)  # fmt: skip
    if rc:
        return code
    assert code == 0, code
    return res
