"""TEST INFRASTRUCTURE: NumPy restatement of jxs_env_select, jxs_env_copy and jxs_env_flags ON THE TILED STORAGE
``[ceil(N/T)][rows][T]`` (flat index arithmetic, padding rule, skip rule), the reference of the host harness
(tests/env_ops_emul.py) and of the device kernels (tests/test_env_ops_gpu.py).  tests/test_env_ops_cpu.py checks it
against plain ``np.where``, fancy indexing and ``np.isfinite`` on untiled ``[rows, N]`` blocks.

Blocks are handled as unsigned integers of the word size, so every bit pattern (NaN payloads, -0, denormals) survives.
"""

from __future__ import annotations

import numpy as np

# (rows, T) of the grid the issue fixes, and the batch sizes per tile
SHAPES = ((5, 32), (155, 2), (38, 4), (1, 64))
FLAG_NONFINITE, FLAG_QUAT_NOT_UNIT = 1, 2


def batch_sizes(T: int) -> list[int]:
    out = []
    for n in (1, T - 1, T, T + 1, 3 * T + 1):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def grid():
    return [(rows, T, N) for rows, T in SHAPES for N in batch_sizes(T)]


def bits_dtype(dtype):
    return {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def n_tiles(N: int, T: int) -> int:
    return -(-N // T)


def storage_words(rows: int, N: int, T: int) -> int:
    return n_tiles(N, T) * rows * T


def random_bits(rng, n: int, dtype) -> np.ndarray:
    """``n`` words of random bit patterns, viewed as ``dtype`` (NaNs, infinities and denormals among them)."""
    u = bits_dtype(dtype)
    return rng.integers(0, np.iinfo(u).max, size=n, dtype=u, endpoint=True).view(dtype)


def word_index(env, row, rows: int, T: int):
    """Flat word of (environment, row) in the storage."""
    env = np.asarray(env, dtype=np.int64)
    return ((env // T) * rows + row) * T + env % T


def word_env(rows: int, N: int, T: int) -> np.ndarray:
    """For every flat word of the storage: the environment of its column (``>= N`` for a padding column)."""
    w = np.arange(storage_words(rows, N, T), dtype=np.int64)
    tile, in_tile = w // (rows * T), w % (rows * T)
    return tile * T + in_tile % T


def select(mask, a: np.ndarray, b: np.ndarray, rows: int, N: int, T: int) -> np.ndarray:
    """out word = a's where the word's column is an environment ``e < N`` with ``mask[e] != 0``, else b's (padding too)."""
    u = bits_dtype(a.dtype)
    mask = np.asarray(mask)
    assert mask.shape == (N,) and a.shape == b.shape == (storage_words(rows, N, T),)
    env = word_env(rows, N, T)
    take = np.zeros(env.shape, dtype=bool)
    real = env < N
    take[real] = mask[env[real]] != 0  # (the mask is never read at or beyond N)
    out = b.view(u).copy()
    out[take] = a.view(u)[take]
    return out.view(a.dtype)


def copy(src: np.ndarray, src_N: int, src_T: int, src_idx, dst: np.ndarray, dst_N: int, dst_T: int, dst_idx, rows: int, K: int) -> np.ndarray:
    """The destination storage after the copy: entry k moves environment ``src_idx[k]`` to ``dst_idx[k]`` (None: k itself);
    an entry with either index outside its block is skipped entirely.  Destinations must be distinct."""
    u = bits_dtype(src.dtype)
    assert src.shape == (storage_words(rows, src_N, src_T),) and dst.shape == (storage_words(rows, dst_N, dst_T),)
    s = np.arange(K, dtype=np.int64) if src_idx is None else np.asarray(src_idx, dtype=np.int64)
    d = np.arange(K, dtype=np.int64) if dst_idx is None else np.asarray(dst_idx, dtype=np.int64)
    ok = (s >= 0) & (s < src_N) & (d >= 0) & (d < dst_N)
    s, d = s[ok], d[ok]
    assert np.unique(d).shape == d.shape, "duplicate destinations are unspecified"
    out = dst.view(u).copy()
    r = np.arange(rows, dtype=np.int64)[:, None]
    out[word_index(d[None, :], r, rows, dst_T)] = src.view(u)[word_index(s[None, :], r, rows, src_T)]
    return out.view(src.dtype)


def flags(state: np.ndarray, rows: int, row_quat: int, N: int, T: int) -> np.ndarray:
    """One byte per environment: bit 0 = a NaN or infinite word, bit 1 = no NaN in the quaternion and its squared norm
    (summed in the block's precision, in row order, from zero) off 1 by more than ``1e-8 + 1e-5``."""
    dt = state.dtype.type
    env = word_env(rows, N, T)
    bad_word = ~np.isfinite(state)
    bad = np.zeros(N, dtype=bool)
    real = env < N
    np.logical_or.at(bad, env[real], bad_word[real])
    e = np.arange(N)
    with np.errstate(all="ignore"):
        q2 = np.zeros(N, dtype=state.dtype)
        nan_q = np.zeros(N, dtype=bool)
        for k in range(4):
            v = state[word_index(e, row_quat + k, rows, T)]
            nan_q |= np.isnan(v)
            q2 = (q2 + v * v).astype(state.dtype)
        d = np.where(q2 > dt(1), q2 - dt(1), dt(1) - q2).astype(state.dtype)
        not_unit = ~nan_q & ~(d <= dt(1e-8) + dt(1e-5))
    return (bad * FLAG_NONFINITE + not_unit * FLAG_QUAT_NOT_UNIT).astype(np.uint8)
