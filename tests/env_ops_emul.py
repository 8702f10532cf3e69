"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the per-environment operations
(tests/emul/jxs_emul_env_ops.cpp), which runs the index functions of jaxsim_amd/csrc/jxs_env_ops.h over every word.

Builds ``tests/emul/libjxs_emul_env_ops.so`` with g++ on demand (a second or two).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
_SRC = _HERE / "emul" / "jxs_emul_env_ops.cpp"
_SO = _HERE / "emul" / "libjxs_emul_env_ops.so"
_ROOT = _HERE.parent
_HEADER = _ROOT / "jaxsim_amd" / "csrc" / "jxs_env_ops.h"


def build(force: bool = False) -> pathlib.Path:
    if force or not _SO.exists() or any(d.stat().st_mtime > _SO.stat().st_mtime for d in (_SRC, _HEADER)):
        tmp = _SO.with_suffix(f".tmp{os.getpid()}.so")
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{_HEADER.parent}", str(_SRC), "-o", str(tmp)]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _SO)
    return _SO


_emul = None


def lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(str(build()))
        vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
        for name, res, argtypes in (("jxs_emul_env_select", i, [vp, vp, vp, vp, i, i, i, i]),
                                    ("jxs_emul_env_copy", i, [vp, i, i, vp, vp, i, i, vp, i, i, i]),
                                    ("jxs_emul_env_flags", i, [vp, i, i, i, i, i, vp]),
                                    ("jxs_emul_env_access_bytes", i, [C.c_ulonglong, i, i, i]),
                                    ("jxs_emul_env_block_words", ll, [i, ll, i]),
                                    ("jxs_emul_env_word_of", ll, [ll, i, i, i])):  # fmt: skip
            getattr(_emul, name).restype = res
            getattr(_emul, name).argtypes = argtypes
    return _emul


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


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
