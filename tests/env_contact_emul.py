"""TEST INFRASTRUCTURE: ctypes binding of the host harness of the contact sensors (tests/emul/jxs_emul_env_contact.cpp), which
runs ``jxs_contact::sense_env`` of jaxsim_amd/csrc/jxs_env_contact.h over every environment of the tiled blocks.

The library is the one of tests/env_emul_lib.py.  A terrain is an ``env_contact_ref.Terrain``, a table an
``env_contact_ref.Table``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from env_emul_lib import _ptr, declare, lib

_vp, _i = C.c_void_p, C.c_int


class TerrainDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("height", C.c_double), ("normal", C.c_double * 3), ("nx", C.c_int32), ("ny", C.c_int32),
                ("origin", C.c_double * 2), ("spacing", C.c_double * 2), ("delta", C.c_double), ("samples", _vp)]  # fmt: skip


declare(("jxs_emul_contact_table_error", _i, [_i, _vp, _i, _vp, _vp, _i, _i, C.POINTER(_i)]),
        ("jxs_emul_env_contacts", _i, [C.POINTER(TerrainDesc), _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, C.c_double, _vp, _vp, _vp, _i]))  # fmt: skip


def _table(tb):
    return (np.ascontiguousarray(tb.groups, dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(tb.parent, dtype=np.int32),
            np.ascontiguousarray(tb.L_p, dtype=np.float64).reshape(-1, 3))  # fmt: skip


def table_error(tb, n_links: int, dtype=np.float32, G=None, P=None) -> tuple[int, int]:
    """``(error code of jxs_contact::table_error, group or entry it is in)``; ``G`` / ``P`` override the counts handed over."""
    g, par, L = _table(tb)
    bad = C.c_int(-1)
    code = lib().jxs_emul_contact_table_error(len(g) if G is None else G, _ptr(g) if g.size else None, len(par) if P is None else P,
                                              _ptr(par) if par.size else None, _ptr(L) if L.size else None, n_links, np.dtype(dtype).itemsize, C.byref(bad))  # fmt: skip
    return code, bad.value


def terrain_desc(tr):
    samples = None if tr.samples is None else np.ascontiguousarray(tr.samples, dtype=np.float64)
    nx, ny = (0, 0) if samples is None else samples.shape
    d = TerrainDesc(tr.kind, tr.height, (C.c_double * 3)(*tr.normal), nx, ny, (C.c_double * 2)(*tr.origin), (C.c_double * 2)(*tr.spacing), tr.delta,
                    None if samples is None else samples.ctypes.data)  # fmt: skip
    return d, samples


def contacts(tr, tb, n_links: int, H: np.ndarray, V, N: int, T: int, dt: float, *, reset=None, timers=None, out=None, rc=False):
    """``(record storage, timer storage or None)`` of the harness.  ``H``, ``V`` (or None), ``timers`` (or None; copied) and
    ``out`` (the words the record holds before the call; copied; default zeros) are flat tiled storages; ``reset`` is ``N`` bytes
    or None.  ``rc=True``: the return code."""
    g, par, L = _table(tb)
    d, keep = terrain_desc(tr)
    dtype = H.dtype
    words = -(-N // T) * T
    res = np.zeros(8 * len(g) * words, dtype) if out is None else np.ascontiguousarray(out).copy()
    tm = None if timers is None else np.ascontiguousarray(timers, dtype=dtype).copy()
    mask = None if reset is None else np.ascontiguousarray(reset, dtype=np.uint8)
    code = lib().jxs_emul_env_contacts(C.byref(d), len(g), _ptr(g), len(par), _ptr(par), _ptr(L), n_links, _ptr(np.ascontiguousarray(H)),
                                       None if V is None else _ptr(np.ascontiguousarray(V, dtype=dtype)), N, T, float(dt), _ptr(mask), _ptr(tm), _ptr(res),
                                       dtype.itemsize)  # fmt: skip
    if rc:
        return code
    assert code == 0, code
    return res, tm
