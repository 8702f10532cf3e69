"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the reward and termination flags
(tests/emul/jxs_emul_env_evaluate.cpp), which runs ``jxs_eval::evaluate_env`` of jaxsim_amd/csrc/jxs_env_evaluate.h over
every environment.

The library is the one of tests/env_emul_lib.py.  A table is an ``env_evaluate_ref.Table``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i, _ll = C.c_void_p, C.c_int, C.c_longlong


class Desc(C.Structure):
    _fields_ = [("D", C.c_int32), ("K", C.c_int32), ("C", C.c_int32), ("slots", _vp), ("targets", _vp), ("offset", _vp), ("scale", _vp),
                ("terms", _vp), ("term_params", _vp), ("conds", _vp), ("cond_limits", _vp), ("reward_lo", C.c_double), ("reward_hi", C.c_double),
                ("termination_reward", C.c_double)]  # fmt: skip


declare(("jxs_emul_evaluate_table_error", _i, [C.POINTER(Desc), _i, _vp, _i, C.POINTER(_i)]),
        ("jxs_emul_evaluate_counted", C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_uint)]),
        ("jxs_emul_env_evaluate", _i, [_vp, _vp, _vp, C.POINTER(Desc), _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _ll, _vp, _i, _i]))  # fmt: skip


def _rows4(source_rows) -> np.ndarray:
    r = np.zeros(4, np.int32)
    if source_rows is not None:
        r[: len(source_rows)] = source_rows
    return r


def desc(tb, D=None, K=None, C_=None):
    """``(Desc, arrays that back its pointers)``; ``D`` / ``K`` / ``C_`` override the counts handed over."""
    keep = [np.ascontiguousarray(tb.slots, dtype=np.int32), np.ascontiguousarray(tb.targets, dtype=np.int32),
            np.ascontiguousarray(tb.offset, dtype=np.float64), np.ascontiguousarray(tb.scale, dtype=np.float64),
            np.ascontiguousarray(tb.terms, dtype=np.int32), np.ascontiguousarray(tb.term_params, dtype=np.float64),
            np.ascontiguousarray(tb.conds, dtype=np.int32), np.ascontiguousarray(tb.cond_limits, dtype=np.float64)]  # fmt: skip
    d = Desc(tb.D if D is None else D, tb.K if K is None else K, tb.C if C_ is None else C_, *[a.ctypes.data if a.size else None for a in keep],
             tb.reward_lo, tb.reward_hi, tb.termination_reward)  # fmt: skip
    return d, keep


def table_error(tb, n_rows: int, source_rows=None, dtype=np.float32, D=None, K=None, C_=None) -> tuple[int, int]:
    d, keep = desc(tb, D, K, C_)
    bad = C.c_int(-1)
    code = lib().jxs_emul_evaluate_table_error(C.byref(d), n_rows, _ptr(_rows4(source_rows)), np.dtype(dtype).itemsize, C.byref(bad))
    return code, bad.value


def counted(steps: int, max_steps: int, done: int) -> tuple[int, int]:
    dn = C.c_uint(done)
    return int(lib().jxs_emul_evaluate_counted(steps, max_steps, C.byref(dn))), dn.value


def evaluate(storage: np.ndarray, tb, n_rows: int, n_joints: int, N: int, T: int, repr_: int, *, sources=(), steps=None, max_steps=0,
             reward=True, done=True, fired=True, terms=True, terms_ld=None, reward_dtype=None, terms_dtype=None, fill=None, rc=False):  # fmt: skip
    """``dict(reward, done, fired, terms [N, terms_ld], steps)`` of the harness; an output switched off is ``None`` (and its
    pointer null).  ``storage``: the tiled state block (flat); ``sources``: up to four tiled blocks as ``(flat storage, rows)`` or
    ``None``; ``steps``: the counters going in (copied); ``fill``: the word the outputs hold before the call (default 0)."""
    dt = storage.dtype
    d, keep_d = desc(tb)
    rdt, tdt = np.dtype(reward_dtype or dt), np.dtype(terms_dtype or dt)
    ld = tb.K if terms_ld is None else int(terms_ld)
    f = 0 if fill is None else fill
    out = dict(reward=np.full(N, f, rdt) if reward else None, done=np.full(N, 0xEE, np.uint8) if done else None,
               fired=np.full(N, 0xEEEEEEEE, np.uint32) if fired else None, terms=np.full((N, ld), f, tdt) if terms else None,
               steps=None if steps is None else np.ascontiguousarray(steps, dtype=np.int32).copy())  # fmt: skip
    keep = [None if x is None else np.ascontiguousarray(x[0], dtype=dt) for x in sources] + [None] * (4 - len(sources))
    ptrs = (C.c_void_p * 4)(*[None if k is None else k.ctypes.data for k in keep])
    rows = _rows4([0 if x is None else x[1] for x in sources])
    code = lib().jxs_emul_env_evaluate(_ptr(np.ascontiguousarray(storage)), ptrs, _ptr(rows), C.byref(d), n_rows, n_joints, int(repr_), N, T,
                                       _ptr(out["reward"]), rdt.itemsize, _ptr(out["done"]), _ptr(out["fired"]), _ptr(out["terms"]), tdt.itemsize, ld,
                                       _ptr(out["steps"]), int(max_steps), dt.itemsize)  # fmt: skip
    if rc:
        return code
    assert code == 0, code
    return out
