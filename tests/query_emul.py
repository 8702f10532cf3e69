"""TEST INFRASTRUCTURE: ctypes binding of the CPU lockstep emulation of the single-launch query modes, MODE_CENTROIDAL,
MODE_FRAMES, MODE_CORIOLIS and MODE_FD_CRB (tests/emul/jxs_emul_query.cpp).

Builds ``tests/emul/libjxs_emul_query.so`` with g++ (``__graft_entry__.build()`` does it next to the main harness).
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
_SRC = _HERE / "emul" / "jxs_emul_query.cpp"
_SO = _HERE / "emul" / "libjxs_emul_query.so"
_ROOT = _HERE.parent
ROWS = 24  # include/jaxsim_amd.h JXS_CENTROIDAL_ROWS and JXS_FRAME_ROWS


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
        _emul.jxs_emul_query_last_error.restype = C.c_char_p
        desc, vp, i = C.POINTER(_lib.ModelDesc), C.c_void_p, C.c_int
        for name, argtypes in (("jxs_emul_centroidal", [desc, vp, vp, vp, i]),
                               ("jxs_emul_frames", [desc, i, vp, vp, vp, i, i, vp, vp, i]),
                               ("jxs_emul_coriolis", [desc, vp, vp, vp, i]),
                               ("jxs_emul_fd_crb", [desc, vp, vp, vp, i, vp, i])):  # fmt: skip
            getattr(_emul, name).restype = C.c_int
            getattr(_emul, name).argtypes = argtypes
    return _emul


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc):
    if rc != 0:
        raise RuntimeError(lib().jxs_emul_query_last_error().decode())


def _setup(model, state, dtype):
    """What every launch starts from: dtype, model description (and what keeps it alive), N, tile, number of tiles and
    the tiled state block."""
    import emul_binding

    dtype = np.dtype(dtype or state.dtype)
    d, keep = _lib.make_desc(model, dtype)
    N = state.shape[1]
    tile = 64 // emul_binding.layout(model, dtype).group
    return dtype, d, keep, N, tile, -(-N // tile), tile_block(np.ascontiguousarray(state, dtype=dtype), tile)


def run_centroidal(model, state: np.ndarray, *, jacobian: bool = True, dtype=None):
    """One emulated launch on a host state block ``[rows, N]``: ``(record [ROWS, N], A_G [6 * (6+n), N] or None)``.
    The outputs start as NaN, so an entry the kernel does not write shows."""
    dtype, d, _keep, N, tile, nt, st = _setup(model, state, dtype)
    n = model.dofs()
    rec = np.full(nt * ROWS * tile, np.nan, dtype=dtype)
    cmm = np.full(nt * 6 * (6 + n) * tile, np.nan, dtype=dtype) if jacobian else None
    _check(lib().jxs_emul_centroidal(C.byref(d), _ptr(st), _ptr(rec), _ptr(cmm), N))
    return untile_block(rec, ROWS, N, tile), (None if cmm is None else untile_block(cmm, 6 * (6 + n), N, tile))


def run_frames(model, state: np.ndarray, parent_links, L_H_F, in_repr: int, out_repr: int, *, jacobian: bool = True, dtype=None):
    """One emulated launch on a host state block ``[rows, N]``: ``(record [N, nt, ROWS], J [N, nt, 6, 6+n] or None)``.
    The outputs start as NaN, so an entry the kernel does not write shows."""
    dtype, d, _keep, N, tile, ntiles, st = _setup(model, state, dtype)
    n = model.dofs()
    parent = np.ascontiguousarray(parent_links, dtype=np.int32).reshape(-1)
    H = np.ascontiguousarray(L_H_F, dtype=np.float64).reshape(-1, 16)
    nt = parent.shape[0]
    rec = np.full(ntiles * nt * ROWS * tile, np.nan, dtype=dtype)
    J = np.full(ntiles * nt * 6 * (6 + n) * tile, np.nan, dtype=dtype) if jacobian else None
    _check(lib().jxs_emul_frames(C.byref(d), nt, _ptr(parent), _ptr(H), _ptr(st), int(in_repr), int(out_repr), _ptr(rec), _ptr(J), N))
    rec_h = untile_block(rec, nt * ROWS, N, tile).T.reshape(N, nt, ROWS)
    J_h = None if J is None else untile_block(J, nt * 6 * (6 + n), N, tile).T.reshape(N, nt, 6, 6 + n)
    return rec_h, J_h


def run_coriolis(model, state: np.ndarray, *, mass_matrix: bool = True, fill=np.nan, dtype=None):
    """One emulated launch on a host state block ``[rows, N]``: ``(C [N, 6+n, 6+n], M [N, 6+n, 6+n] or None)``, Mixed.
    The outputs start as ``fill``: NaN shows the entries the kernel writes, 0 is what ``jxs_coriolis`` hands it."""
    dtype, d, _keep, N, tile, ntiles, st = _setup(model, state, dtype)
    nv = 6 + model.dofs()
    Cm = np.full(ntiles * nv * nv * tile, fill, dtype=dtype)
    M = np.full(ntiles * nv * nv * tile, fill, dtype=dtype) if mass_matrix else None
    _check(lib().jxs_emul_coriolis(C.byref(d), _ptr(st), _ptr(Cm), _ptr(M), N))
    C_h = untile_block(Cm, nv * nv, N, tile).T.reshape(N, nv, nv)
    M_h = None if M is None else untile_block(M, nv * nv, N, tile).T.reshape(N, nv, nv)
    return C_h, M_h


def run_fd_crb(model, state: np.ndarray, *, tau=None, link_forces=None, force_repr: int = 0, fill=np.nan, dtype=None) -> np.ndarray:
    """One emulated launch on a host state block ``[rows, N]``: the accelerations ``[6+n, N]`` (inertial-fixed base
    acceleration, then the joint accelerations).  ``tau`` is ``[n, N]``, ``link_forces`` ``[nL * 6, N]`` in ``force_repr``
    (0 inertial, 1 body, 2 mixed).  The output starts as ``fill``: NaN shows that the kernel writes every entry."""
    dtype, d, _keep, N, tile, ntiles, st = _setup(model, state, dtype)
    nv = 6 + model.dofs()

    def up(a):
        return None if a is None else tile_block(np.ascontiguousarray(a, dtype=dtype), tile)

    tq, lf = up(tau), up(link_forces)
    out = np.full(ntiles * nv * tile, fill, dtype=dtype)
    _check(lib().jxs_emul_fd_crb(C.byref(d), _ptr(st), _ptr(tq), _ptr(lf), int(force_repr), _ptr(out), N))
    return untile_block(out, nv, N, tile)
