"""Host NumPy form of the random-reset sampler of the device (``csrc/jxs_env_random.h``): Philox4x32-10 and the uniform
variables drawn from it, bit for bit what ``jxs_env_randomize`` draws.

A value depends on ``(seed, draw, global environment, variable)`` only: key = (seed low, seed high), counter = (global
environment, variable, draw low, draw high), one block per variable, output words 0 and 1 used."""

from __future__ import annotations

import numpy as np

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """Four arrays of 32-bit output words (as uint64) for four counter and two key words, broadcast against each other."""
    c = list(np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _LOW for x in counter]))
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _LOW for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # (32 x 32 -> 64 bits: exact)
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & _LOW, (p0 >> _32) ^ c[3] ^ k1, p0 & _LOW]
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return c


def unit_uniform(env_global, variable, seed: int, draw: int, dtype) -> np.ndarray:
    """``u`` in [0, 1): ``(w0 >> 8) 2^-24`` in float32, ``((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53`` in float64."""
    seed, draw = int(seed), int(draw)
    if not (0 <= seed < 2**64 and 0 <= draw < 2**64):
        raise ValueError("seed and draw must fit 64 unsigned bits")
    w = philox4x32_10((env_global, variable, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    if np.dtype(dtype) == np.float32:
        return (w[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
    return (((w[0] >> np.uint64(5)) << np.uint64(26)) + (w[1] >> np.uint64(6))).astype(np.float64) * 2.0**-53


def uniform(lo, hi, env_global, variable, seed: int, draw: int) -> np.ndarray:
    """``lo + u (hi - lo)`` in the dtype of ``lo``, every operation rounded on its own, clamped from above."""
    lo = np.asarray(lo)
    dt = lo.dtype
    hi = np.asarray(hi, dtype=dt)
    u = unit_uniform(env_global, variable, seed, draw, dt)
    x = (lo + (u * (hi - lo).astype(dt)).astype(dt)).astype(dt)
    return np.where(x > hi, hi, x).astype(dt)
