"""TEST INFRASTRUCTURE: ctypes binding of the CPU lockstep emulation of MODE_FRAMES (tests/emul/jxs_emul_frames.cpp).

Builds ``tests/emul/libjxs_emul_frames.so`` with g++ (``__graft_entry__.build()`` does it next to the main harness).
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
_SRC = _HERE / "emul" / "jxs_emul_frames.cpp"
_SO = _HERE / "emul" / "libjxs_emul_frames.so"
_ROOT = _HERE.parent
ROWS = 24  # include/jaxsim_amd.h JXS_FRAME_ROWS


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
        _emul.jxs_emul_frames_last_error.restype = C.c_char_p
        vp = C.c_void_p
        _emul.jxs_emul_frames.restype = C.c_int
        _emul.jxs_emul_frames.argtypes = [C.POINTER(_lib.ModelDesc), C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int]
    return _emul


def run(model, state: np.ndarray, parent_links, L_H_F, in_repr: int, out_repr: int, *, jacobian: bool = True, dtype=None):
    """One emulated launch on a host state block ``[rows, N]``: ``(record [N, nt, ROWS], J [N, nt, 6, 6+n] or None)``.
    The outputs start as NaN, so an entry the kernel does not write shows."""
    import emul_binding

    dtype = np.dtype(dtype or state.dtype)
    d, _keep = _lib.make_desc(model, dtype)
    N, n = state.shape[1], model.dofs()
    parent = np.ascontiguousarray(parent_links, dtype=np.int32).reshape(-1)
    H = np.ascontiguousarray(L_H_F, dtype=np.float64).reshape(-1, 16)
    nt = parent.shape[0]
    tile = 64 // emul_binding.layout(model, dtype).group
    ntiles = -(-N // tile)
    st = tile_block(np.ascontiguousarray(state, dtype=dtype), tile)
    rec = np.full(ntiles * nt * ROWS * tile, np.nan, dtype=dtype)
    J = np.full(ntiles * nt * 6 * (6 + n) * tile, np.nan, dtype=dtype) if jacobian else None
    rc = lib().jxs_emul_frames(C.byref(d), nt, parent.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p),
                               st.ctypes.data_as(C.c_void_p), int(in_repr), int(out_repr), rec.ctypes.data_as(C.c_void_p),
                               None if J is None else J.ctypes.data_as(C.c_void_p), N)  # fmt: skip
    if rc != 0:
        raise RuntimeError(lib().jxs_emul_frames_last_error().decode())
    rec_h = untile_block(rec, nt * ROWS, N, tile).T.reshape(N, nt, ROWS)
    J_h = None if J is None else untile_block(J, nt * 6 * (6 + n), N, tile).T.reshape(N, nt, 6, 6 + n)
    return rec_h, J_h
