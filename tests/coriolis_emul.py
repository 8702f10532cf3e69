"""TEST INFRASTRUCTURE: ctypes binding of the CPU lockstep emulation of MODE_CORIOLIS (tests/emul/jxs_emul_coriolis.cpp).

Builds ``tests/emul/libjxs_emul_coriolis.so`` with g++ (``__graft_entry__.build()`` does it next to the main harness).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

import numpy as np

from jaxsim_amd import _lib
from jaxsim_amd.state import tile_block, untile_block

_HERE = pathlib.Path(__file__).resolve().parent
_SRC = _HERE / "emul" / "jxs_emul_coriolis.cpp"
_SO = _HERE / "emul" / "libjxs_emul_coriolis.so"
_ROOT = _HERE.parent


def build(force: bool = False) -> pathlib.Path:
    deps = [_SRC, _HERE / "emul" / "jxs_lanes_host.h", _ROOT / "include" / "jaxsim_amd.h"]
    deps += sorted((_ROOT / "jaxsim_amd" / "csrc").glob("*.h")) + sorted((_ROOT / "jaxsim_amd" / "csrc").glob("*.inc"))
    if force or not _SO.exists() or any(d.stat().st_mtime > _SO.stat().st_mtime for d in deps):
        tmp = _SO.with_suffix(f".tmp{os.getpid()}.so")
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", f"-I{_ROOT / 'jaxsim_amd' / 'csrc'}",
               f"-I{_HERE / 'emul'}", str(_SRC), "-o", str(tmp)]  # fmt: skip
        subprocess.run(cmd, check=True)
        os.replace(tmp, _SO)
    return _SO


_emul = None


def lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(str(build()))
        _emul.jxs_emul_coriolis_last_error.restype = C.c_char_p
        vp = C.c_void_p
        _emul.jxs_emul_coriolis.restype = C.c_int
        _emul.jxs_emul_coriolis.argtypes = [C.POINTER(_lib.ModelDesc), vp, vp, vp, C.c_int]
    return _emul


def run(model, state: np.ndarray, *, mass_matrix: bool = True, fill=np.nan, dtype=None):
    """One emulated launch on a host state block ``[rows, N]``: ``(C [N, 6+n, 6+n], M [N, 6+n, 6+n] or None)``, Mixed.
    The outputs start as ``fill``: NaN shows the entries the kernel writes, 0 is what ``jxs_coriolis`` hands it."""
    import emul_binding

    dtype = np.dtype(dtype or state.dtype)
    d, _keep = _lib.make_desc(model, dtype)
    N, nv = state.shape[1], 6 + model.dofs()
    tile = 64 // emul_binding.layout(model, dtype).group
    ntiles = -(-N // tile)
    st = tile_block(np.ascontiguousarray(state, dtype=dtype), tile)
    Cm = np.full(ntiles * nv * nv * tile, fill, dtype=dtype)
    M = np.full(ntiles * nv * nv * tile, fill, dtype=dtype) if mass_matrix else None
    rc = lib().jxs_emul_coriolis(C.byref(d), st.ctypes.data_as(C.c_void_p), Cm.ctypes.data_as(C.c_void_p),
                                 None if M is None else M.ctypes.data_as(C.c_void_p), N)  # fmt: skip
    if rc != 0:
        raise RuntimeError(lib().jxs_emul_coriolis_last_error().decode())
    C_h = untile_block(Cm, nv * nv, N, tile).T.reshape(N, nv, nv)
    M_h = None if M is None else untile_block(M, nv * nv, N, tile).T.reshape(N, nv, nv)
    return C_h, M_h
