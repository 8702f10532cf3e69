"""TEST INFRASTRUCTURE: the one shared library of the host harnesses of the per-environment operations
(tests/emul/jxs_emul_env_*.cpp), which run the functions of jaxsim_amd/csrc/jxs_env_*.h over every word on the CPU.  The
domain wrappers are env_ops_emul.py, env_random_emul.py, env_observe_emul.py and env_act_emul.py.

Builds ``tests/emul/libjxs_emul_env.so`` with g++ on demand (a few seconds).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

_HERE = pathlib.Path(__file__).resolve().parent
_SO = _HERE / "emul" / "libjxs_emul_env.so"
_CSRC = _HERE.parent / "jaxsim_amd" / "csrc"


def _sources() -> list[pathlib.Path]:
    return sorted((_HERE / "emul").glob("jxs_emul_env_*.cpp"))


def build(force: bool = False) -> pathlib.Path:
    deps = _sources() + sorted(_CSRC.glob("jxs_env_*.h"))
    if force or not _SO.exists() or any(d.stat().st_mtime > _SO.stat().st_mtime for d in deps):
        tmp = _SO.with_suffix(f".tmp{os.getpid()}.so")
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", f"-I{_CSRC}", *map(str, _sources()), "-o", str(tmp)]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _SO)
    return _SO


_emul = None
_pending = []


def declare(*signatures) -> None:
    """``(name, restype, argtypes)`` of the functions a wrapper module calls: set on the library when it is next asked for."""
    _pending.extend(signatures)


def lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(str(build()))
    while _pending:
        name, res, argtypes = _pending.pop()
        f = getattr(_emul, name)
        f.restype, f.argtypes = res, argtypes
    return _emul


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)
