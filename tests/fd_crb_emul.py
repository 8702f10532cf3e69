"""TEST INFRASTRUCTURE: ctypes binding of the CPU lockstep emulation of MODE_FD_CRB (tests/emul/jxs_emul_fd_crb.cpp).

Builds ``tests/emul/libjxs_emul_fd_crb.so`` with g++ (``__graft_entry__.build()`` does it next to the main harness).
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
_SRC = _HERE / "emul" / "jxs_emul_fd_crb.cpp"
_SO = _HERE / "emul" / "libjxs_emul_fd_crb.so"
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
        _emul.jxs_emul_fd_crb_last_error.restype = C.c_char_p
        vp = C.c_void_p
        _emul.jxs_emul_fd_crb.restype = C.c_int
        _emul.jxs_emul_fd_crb.argtypes = [C.POINTER(_lib.ModelDesc), vp, vp, vp, C.c_int, vp, C.c_int]
    return _emul


def run(model, state: np.ndarray, *, tau=None, link_forces=None, force_repr: int = 0, fill=np.nan, dtype=None) -> np.ndarray:
    """One emulated launch on a host state block ``[rows, N]``: the accelerations ``[6+n, N]`` (inertial-fixed base
    acceleration, then the joint accelerations).  ``tau`` is ``[n, N]``, ``link_forces`` ``[nL * 6, N]`` in ``force_repr``
    (0 inertial, 1 body, 2 mixed).  The output starts as ``fill``: NaN shows that the kernel writes every entry."""
    import emul_binding

    dtype = np.dtype(dtype or state.dtype)
    d, _keep = _lib.make_desc(model, dtype)
    N, nv = state.shape[1], 6 + model.dofs()
    tile = 64 // emul_binding.layout(model, dtype).group
    ntiles = -(-N // tile)

    def up(a):
        return None if a is None else tile_block(np.ascontiguousarray(a, dtype=dtype), tile)

    def p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    st, tq, lf = up(state), up(tau), up(link_forces)
    out = np.full(ntiles * nv * tile, fill, dtype=dtype)
    rc = lib().jxs_emul_fd_crb(C.byref(d), p(st), p(tq), p(lf), int(force_repr), p(out), N)
    if rc != 0:
        raise RuntimeError(lib().jxs_emul_fd_crb_last_error().decode())
    return untile_block(out, nv, N, tile)
