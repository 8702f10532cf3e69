"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the per-environment operations
(tests/emul/jxs_emul_env_ops.cpp), which runs the index functions of jaxsim_amd/csrc/jxs_env_ops.h over every word.
The library is the one of tests/env_emul_lib.py.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
declare(("jxs_emul_env_select", _i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i]),
        ("jxs_emul_env_copy", _i, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _i, _i]),
        ("jxs_emul_env_flags", _i, [_vp, _i, _i, _i, _i, _i, _vp]),
        ("jxs_emul_env_access_bytes", _i, [C.c_ulonglong, _i, _i, _i]),
        ("jxs_emul_env_shift_for", _i, [_i, _i, _i]),
        ("jxs_emul_env_block_words", _ll, [_i, _ll, _i]),
        ("jxs_emul_env_word_of", _ll, [_ll, _i, _i, _i]))  # fmt: skip


def select(mask, a: np.ndarray, b: np.ndarray, rows: int, N: int, T: int, *, out: np.ndarray | None = None) -> np.ndarray:
    """``out`` may be ``a`` or ``b`` themselves (the aliasing the entry point allows); a new array otherwise."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    if out is None:
        out = np.empty_like(b)
    assert lib().jxs_emul_env_select(_ptr(mask), _ptr(a), _ptr(b), _ptr(out), rows, N, T, a.dtype.itemsize) == 0
    return out


def copy(src: np.ndarray, src_N: int, src_T: int, src_idx, dst: np.ndarray, dst_N: int, dst_T: int, dst_idx, rows: int, K: int) -> np.ndarray:
    """The destination storage after the copy (``dst`` itself is left alone)."""
    si = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int32)
    di = None if dst_idx is None else np.ascontiguousarray(dst_idx, dtype=np.int32)
    out = dst.copy()
    rc = lib().jxs_emul_env_copy(_ptr(src), src_N, src_T, _ptr(si), _ptr(out), dst_N, dst_T, _ptr(di), rows, K, src.dtype.itemsize)
    assert rc == 0, f"jxs_emul_env_copy: {rc} (-2: a word outside its block)"
    return out


def flags(state: np.ndarray, rows: int, row_quat: int, N: int, T: int) -> np.ndarray:
    out = np.full(N, 0xFF, dtype=np.uint8)
    assert lib().jxs_emul_env_flags(_ptr(state), rows, row_quat, N, T, state.dtype.itemsize, _ptr(out)) == 0
    return out


def access_bytes(address_bits: int, rows: int, T: int, word_bytes: int) -> int:
    return lib().jxs_emul_env_access_bytes(address_bits, rows, T, word_bytes)


def env_shift_for(N: int, tile_shift: int, want: int = 0) -> int:
    return lib().jxs_emul_env_shift_for(N, tile_shift, want)
