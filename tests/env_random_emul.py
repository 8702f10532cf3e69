"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the random reset (tests/emul/jxs_emul_env_random.cpp),
which runs the functions of jaxsim_amd/csrc/jxs_env_random.h over every word of a block.

Builds ``tests/emul/libjxs_emul_env_random.so`` with g++ on demand (a second or two).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
_SRC = _HERE / "emul" / "jxs_emul_env_random.cpp"
_SO = _HERE / "emul" / "libjxs_emul_env_random.so"
_CSRC = _HERE.parent / "jaxsim_amd" / "csrc"
_HEADERS = (_CSRC / "jxs_env_random.h", _CSRC / "jxs_env_ops.h")


def build(force: bool = False) -> pathlib.Path:
    if force or not _SO.exists() or any(d.stat().st_mtime > _SO.stat().st_mtime for d in (_SRC, *_HEADERS)):
        tmp = _SO.with_suffix(f".tmp{os.getpid()}.so")
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", f"-I{_CSRC}", str(_SRC), "-o", str(tmp)]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _SO)
    return _SO


_emul = None


def lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(str(build()))
        vp, i, u64 = C.c_void_p, C.c_int, C.c_uint64
        _emul.jxs_emul_philox4x32_10.restype = None
        _emul.jxs_emul_philox4x32_10.argtypes = [vp, vp, vp]
        _emul.jxs_emul_env_randomize.restype = i
        _emul.jxs_emul_env_randomize.argtypes = [vp, vp, i, i, i, i, i, i, vp, u64, u64, C.c_longlong, i]
        _emul.jxs_emul_env_random_variables.restype = i
        _emul.jxs_emul_env_random_variables.argtypes = [i]
    return _emul


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def philox(ctr, key) -> tuple:
    c, k, out = np.asarray(ctr, dtype=np.uint32), np.asarray(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    lib().jxs_emul_philox4x32_10(_ptr(c), _ptr(k), _ptr(out))
    return tuple(int(x) for x in out)


def randomize(storage: np.ndarray, mask, n: int, n_points: int, N: int, T: int, bounds: np.ndarray, seed=0, draw=0, first_env=0,
              floating=True, repr_=2, *, rc=False):  # fmt: skip
    """The tiled storage after the reset (``storage`` itself is left alone).  ``rc=True``: the return code instead."""
    out = np.ascontiguousarray(storage).copy()
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    b = np.ascontiguousarray(bounds, dtype=storage.dtype)
    assert b.shape == (2, lib().jxs_emul_env_random_variables(n))
    code = lib().jxs_emul_env_randomize(_ptr(m), _ptr(out), 13 + 2 * n + 3 * n_points, N, T, n, int(floating), int(repr_), _ptr(b),
                                        seed, draw, first_env, storage.dtype.itemsize)  # fmt: skip
    if rc:
        return code
    assert code == 0, code
    return out
