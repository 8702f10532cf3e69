"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the random reset (tests/emul/jxs_emul_env_random.cpp),
which runs the functions of jaxsim_amd/csrc/jxs_env_random.h over every word of a block.

The library is the one of tests/env_emul_lib.py.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i, _u64 = C.c_void_p, C.c_int, C.c_uint64
declare(("jxs_emul_philox4x32_10", None, [_vp, _vp, _vp]),
        ("jxs_emul_env_randomize", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _u64, _u64, C.c_longlong, _i]),
        ("jxs_emul_env_random_variables", _i, [_i]))  # fmt: skip


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
