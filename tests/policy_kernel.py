"""TEST INFRASTRUCTURE: ctypes binding of the stand-in policy of tests/test_env_observe_gpu.py
(tests/emul/jxs_test_policy.hip): a PD torque computed on the device from an observation tensor, by code that is not part
of the product -- what another framework's network is to the loop step -> observe -> policy -> step.

Builds ``tests/emul/libjxs_test_policy.so`` with hipcc for gfx950 on demand (``__graft_entry__.build()`` builds it ahead).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

_HERE = pathlib.Path(__file__).resolve().parent
_SRC = _HERE / "emul" / "jxs_test_policy.hip"
_SO = _HERE / "emul" / "libjxs_test_policy.so"


def build(force: bool = False) -> pathlib.Path:
    if force or not _SO.exists() or _SRC.stat().st_mtime > _SO.stat().st_mtime:
        tmp = _SO.with_suffix(f".tmp{os.getpid()}.so")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", str(_SRC), "-o", str(tmp)]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _SO)
    return _SO


_policy = None


def lib():
    global _policy
    if _policy is None:
        _policy = C.CDLL(str(build()))
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        _policy.jxs_test_pd_torque.restype = i
        _policy.jxs_test_pd_torque.argtypes = [vp, C.c_longlong, vp, i, i, f, f, vp, vp]
    return _policy


def pd_torque(obs_ptr: int, ld: int, q0_ptr: int, n: int, N: int, kp: float, kd: float, tau_ptr: int, stream) -> None:
    """tau[N][n] = (q0 - obs[:, :n]) * kp - obs[:, n:2n] * kd in float32, asynchronous on ``stream`` (a handle or None)."""
    rc = lib().jxs_test_pd_torque(C.c_void_p(obs_ptr), ld, C.c_void_p(q0_ptr), n, N, kp, kd, C.c_void_p(tau_ptr), stream)
    assert rc == 0, rc
