"""TEST INFRASTRUCTURE: NumPy restatement of the random reset (jxs_env_randomize), written from its specification and
importing nothing of the product: Philox4x32-10, the uniform variables, the rows of the state block on the tiled
storage ``[ceil(N/T)][rows][T]``.  The reference of the host harness (tests/env_random_emul.py) and of the device kernel
(tests/test_env_random_gpu.py).

A value depends on ``(seed, draw, first_env + e, variable)`` only.  Key = (seed low, seed high); counter = (global
environment, variable, draw low, draw high); one block per variable, words 0 and 1 used.  Variables of a model with n
joints: 0-2 position, 3-5 XYZ Euler angles, 6..5+n joint positions, 6+n..8+n linear, 9+n..11+n angular base velocity,
12+n..11+2n joint velocities.  Rows: jaxsim_amd/state.py.

Rows that are a variable or a zero are restated in the block's dtype and are compared bitwise; the quaternion and the
Mixed / Body velocity rows involve sines, cosines and products, they are restated in float64 (``exact_rows``) and
compared within the tolerances the tests state.
"""

from __future__ import annotations

import numpy as np

import env_ops_ref as eref

INERTIAL, BODY, MIXED = 0, 1, 2
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

# (counter, key) -> output, the known answers of Philox4x32-10
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(ctr, key):
    """``ctr``: four, ``key``: two broadcastable arrays of 32-bit words.  Four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & MASK32 for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # (32 x 32 bits: no overflow in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return [x.astype(np.uint32) for x in c]


def n_variables(n: int) -> int:
    return 12 + 2 * n


def n_rows(n: int, n_points: int) -> int:
    return 13 + 2 * n + 3 * n_points


def unit_uniform(env_global, v, seed: int, draw: int, dtype):
    """u in [0, 1) of variable(s) ``v`` of the global environment(s), exact in ``dtype``."""
    w = philox4x32_10((env_global, v, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    w0, w1 = w[0].astype(np.uint64), w[1].astype(np.uint64)
    if np.dtype(dtype) == np.float32:
        return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
    return (((w0 >> np.uint64(5)) << np.uint64(26)) + (w1 >> np.uint64(6))).astype(np.float64) * 2.0**-53


def variables(bounds: np.ndarray, env_global, seed: int, draw: int) -> np.ndarray:
    """``[nv, E]`` values of all variables: ``lo + u * (hi - lo)``, each operation rounded in the dtype of ``bounds``
    (NumPy rounds every array operation on its own), clamped from above."""
    dt = bounds.dtype
    nv = bounds.shape[1]
    env_global = np.asarray(env_global, dtype=np.uint64).reshape(1, -1)
    u = unit_uniform(env_global, np.arange(nv, dtype=np.uint64).reshape(-1, 1), seed, draw, dt)
    lo, hi = bounds[0].reshape(-1, 1), bounds[1].reshape(-1, 1)
    d = (hi - lo).astype(dt)
    m = (u * d).astype(dt)
    x = (lo + m).astype(dt)
    return np.where(x > hi, hi, x).astype(dt)


def quaternion_of_euler_xyz(a):
    """wxyz of Rx(a0) Ry(a1) Rz(a2), float64; ``a``: [3, E]."""
    h = np.asarray(a, dtype=np.float64) / 2
    (sx, sy, sz), (cx, cy, cz) = np.sin(h), np.cos(h)
    return np.stack([cx * cy * cz - sx * sy * sz, sx * cy * cz + cx * sy * sz, cx * sy * cz - sx * cy * sz, cx * cy * sz + sx * sy * cz])


def rotation_of_quaternion(q):
    """[E, 3, 3] of wxyz ``q`` [4, E] (normalised first), float64."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q, axis=0, keepdims=True)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])  # fmt: skip
    return np.moveaxis(R, -1, 0)


class Rows:
    """Which rows of a block of n joints and n_points points are what."""

    def __init__(self, n: int, n_points: int):
        self.n, self.n_points, self.rows = n, n_points, n_rows(n, n_points)
        self.pos, self.quat, self.s, self.vlin, self.vang, self.sd, self.m = 0, 3, 7, 7 + n, 10 + n, 13 + n, 13 + 2 * n

    def bitwise(self, floating: bool, repr_: int) -> np.ndarray:
        """Rows whose words are a variable or a zero: bitwise equal to ``sampled_block``."""
        r = np.ones(self.rows, dtype=bool)
        r[self.quat : self.quat + 4] = False
        if floating and repr_ != INERTIAL:
            r[self.vlin : self.vlin + 3] = False
            if repr_ == BODY:
                r[self.vang : self.vang + 3] = False
        return r


def sampled_block(n: int, n_points: int, bounds: np.ndarray, env_global, seed: int, draw: int, floating: bool, repr_: int):
    """``(block [rows, E] in the dtype of bounds, exact [rows, E] float64)`` of the environments ``env_global``.

    ``block`` holds the rows that are a variable or a zero (bitwise what the kernel writes) and, in the other rows, the
    float64 restatement rounded to the dtype; ``exact`` is the float64 restatement evaluated on the bitwise-known
    variables: the quaternion of the sampled angles, the velocity rows from the sampled (l, a), the sampled p and the
    rotation of that quaternion."""
    L = Rows(n, n_points)
    dt = bounds.dtype
    x = variables(bounds, env_global, seed, draw)
    E = x.shape[1]
    blk = np.zeros((L.rows, E), dtype=dt)
    blk[0:3] = x[0:3]
    blk[L.s : L.s + n] = x[6 : 6 + n]
    blk[L.sd : L.sd + n] = x[12 + n : 12 + 2 * n]
    exact = blk.astype(np.float64)
    q = quaternion_of_euler_xyz(x[3:6])
    exact[L.quat : L.quat + 4] = q
    if floating:
        lin, ang = x[6 + n : 9 + n].astype(np.float64), x[9 + n : 12 + n].astype(np.float64)
        if repr_ == INERTIAL:
            blk[L.vlin : L.vlin + 3], blk[L.vang : L.vang + 3] = x[6 + n : 9 + n], x[9 + n : 12 + n]
            exact[L.vlin : L.vang + 3] = np.concatenate([lin, ang])
        else:
            if repr_ == BODY:
                R = rotation_of_quaternion(q)
                lin, ang = np.einsum("eij,je->ie", R, lin), np.einsum("eij,je->ie", R, ang)
            else:
                blk[L.vang : L.vang + 3] = x[9 + n : 12 + n]
            p = x[0:3].astype(np.float64)
            exact[L.vlin : L.vlin + 3] = lin + np.cross(p, ang, axis=0)
            exact[L.vang : L.vang + 3] = ang
    rounded = ~L.bitwise(floating, repr_)
    blk[rounded] = exact[rounded].astype(dt)
    return blk, exact


def velocity_of_block(L: Rows, blk: np.ndarray, lin, ang, repr_: int) -> np.ndarray:
    """The six stored base-velocity rows, float64, from the sampled (l, a) and the BLOCK's own p and q."""
    p = blk[0:3].astype(np.float64)
    lin, ang = np.asarray(lin, dtype=np.float64), np.asarray(ang, dtype=np.float64)
    if repr_ == BODY:
        R = rotation_of_quaternion(blk[L.quat : L.quat + 4])
        lin, ang = np.einsum("eij,je->ie", R, lin), np.einsum("eij,je->ie", R, ang)
    return np.concatenate([lin + np.cross(p, ang, axis=0), ang])


def mask_envs(mask, N: int) -> np.ndarray:
    return np.ones(N, dtype=bool) if mask is None else np.asarray(mask)[:N] != 0


def randomize(storage: np.ndarray, mask, n: int, n_points: int, N: int, T: int, bounds, seed, draw, first_env, floating, repr_):
    """The tiled storage after the reset: the words of the environments the mask names (all of them for ``None``) come
    from ``sampled_block``, every other word -- the other environments, the padding columns -- keeps its bits.  Returns
    ``(storage, exact [rows, N] float64, taken [N] bool)``."""
    L = Rows(n, n_points)
    assert storage.shape == (eref.storage_words(L.rows, N, T),) and storage.dtype == bounds.dtype
    u = eref.bits_dtype(storage.dtype)
    take = mask_envs(mask, N)
    blk, exact = sampled_block(n, n_points, bounds, first_env + np.arange(N), seed, draw, floating, repr_)
    out = storage.view(u).copy()
    e = np.nonzero(take)[0]
    r = np.arange(L.rows).reshape(-1, 1)
    out[eref.word_index(e.reshape(1, -1), r, L.rows, T)] = blk.view(u)[:, e]
    return out.view(storage.dtype), exact, take


def untile(storage: np.ndarray, rows: int, N: int, T: int) -> np.ndarray:
    """[rows, N] view of the environments of a tiled storage (a copy; padding dropped)."""
    nt = eref.n_tiles(N, T)
    return np.ascontiguousarray(storage.reshape(nt, rows, T).transpose(1, 0, 2).reshape(rows, nt * T)[:, :N])


def default_bounds(n: int, dtype, rng=None) -> np.ndarray:
    """A bounds table [2][12 + 2n]: the defaults of the reference, or random intervals."""
    nv = n_variables(n)
    lo, hi = -np.ones(nv), np.ones(nv)
    lo[0:3], hi[0:3] = (-1, -1, 0.5), (1, 1, 1)
    lo[3:6], hi[3:6] = -np.pi, np.pi
    if rng is not None:
        lo[6:] = rng.uniform(-3, 1, nv - 6)
        hi[6:] = lo[6:] + rng.uniform(0, 4, nv - 6)
    return np.stack([lo, hi]).astype(dtype)
