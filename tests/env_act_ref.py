"""TEST INFRASTRUCTURE: NumPy restatement of the action-to-torque law (``jxs_env_act``), written from the formula in
include/jaxsim_amd.h; it does not import the product.

``act(q, qd, ...)`` evaluates every joint of every environment on logical ``[n, N]`` arrays of the block's dtype: one NumPy
operation per rounding, ``np.where`` chains for ``clamp``.  Only ``+ - x`` and comparisons are involved, so the result is
comparable bit for bit.
"""

from __future__ import annotations

import numpy as np

OFF, TORQUE, POSITION, VELOCITY = range(4)
SCALE, OFFSET, KP, KD, ACTION_CLIP, TARGET_LO, TARGET_HI, TORQUE_LIMIT = range(8)
MAX_WIDTH = 4096
# error codes of the validity check
OK, BAD_JOINTS, BAD_WIDTH, BAD_MODE, BAD_COLUMN, NOT_FINITE, BAD_LIMIT, BAD_TARGETS = range(8)


def n_rows(n_joints: int, n_points: int) -> int:
    return 13 + 2 * n_joints + 3 * n_points


def row_q(n_joints: int) -> int:
    return 7


def row_qd(n_joints: int) -> int:
    return 13 + n_joints


def tile_block(block: np.ndarray, T: int, pad=0.0) -> np.ndarray:
    """``[rows, N]`` -> the flat storage ``[ceil(N/T)][rows][T]``; the padding columns hold ``pad``."""
    rows, N = block.shape
    nt = -(-N // T)
    wide = np.full((rows, nt * T), pad, dtype=block.dtype)
    wide[:, :N] = block
    return np.ascontiguousarray(wide.reshape(rows, nt, T).transpose(1, 0, 2)).reshape(-1)


def untile_block(flat: np.ndarray, rows: int, N: int, T: int) -> tuple[np.ndarray, np.ndarray]:
    """The flat storage -> ``([rows, N], the padding columns [rows, nt * T - N])``."""
    nt = -(-N // T)
    wide = flat.reshape(nt, rows, T).transpose(1, 0, 2).reshape(rows, nt * T)
    return np.ascontiguousarray(wide[:, :N]), np.ascontiguousarray(wide[:, N:])


def clamp(x, lo, hi):
    """``x < lo ? lo : (hi < x ? hi : x)``: a NaN x passes through, -0 keeps its sign."""
    with np.errstate(invalid="ignore"):
        return np.where(x < lo, lo, np.where(hi < x, hi, x))


def finite_in(v: float, dtype) -> bool:
    with np.errstate(over="ignore"):
        return bool(np.isfinite(v) and np.isfinite(np.asarray(v, np.float64).astype(dtype)))


def limit_ok(v: float, dtype) -> bool:
    return bool(v >= 0) and (np.isposinf(v) or finite_in(v, dtype))


def targets_ok(lo: float, hi: float, dtype) -> bool:
    return bool(lo <= hi) and all(np.isinf(v) or finite_in(v, dtype) for v in (lo, hi))


def table_error(joints, params, A: int, dtype, n=None) -> tuple[int, int]:
    """``(code, joint)`` of the first refusal of a table, ``(OK, -1)`` for a valid one."""
    joints, params = np.asarray(joints, np.int64).reshape(-1, 2), np.asarray(params, np.float64).reshape(-1, 8)
    n = len(joints) if n is None else n
    if n < 1:
        return BAD_JOINTS, -1
    if A < 0 or A > MAX_WIDTH:
        return BAD_WIDTH, -1
    for j in range(n):
        (mode, column), p = joints[j], params[j]
        if not OFF <= mode <= VELOCITY:
            return BAD_MODE, j
        if not -1 <= column < A:
            return BAD_COLUMN, j
        if not all(finite_in(p[k], dtype) for k in (SCALE, OFFSET, KP, KD)):
            return NOT_FINITE, j
        if not (limit_ok(p[ACTION_CLIP], dtype) and limit_ok(p[TORQUE_LIMIT], dtype)):
            return BAD_LIMIT, j
        if not targets_ok(p[TARGET_LO], p[TARGET_HI], dtype):
            return BAD_TARGETS, j
    return OK, -1


def act(q: np.ndarray, qd: np.ndarray, joints, params, actions, feed_forward=None) -> np.ndarray:
    """``tau [n, N]`` in the dtype of ``q``.  ``q`` / ``qd`` / ``feed_forward``: ``[n, N]``; ``actions``: ``[N, >= A]`` of
    float32 or that dtype, or ``None`` when no joint has a column; ``params`` ``[n, 8]`` float64, rounded to the dtype here."""
    dt = q.dtype
    n, N = q.shape
    joints = np.asarray(joints, np.int64).reshape(n, 2)
    with np.errstate(over="ignore"):
        P = np.asarray(params, np.float64).reshape(n, 8).astype(dt)
    out = np.empty((n, N), dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            mode, column = int(joints[j, 0]), int(joints[j, 1])
            p = P[j]
            a = np.zeros(N, dt) if column < 0 else np.asarray(actions)[:, column].astype(dt)
            prod = clamp(a, -p[ACTION_CLIP], p[ACTION_CLIP]) * p[SCALE]
            u = prod + p[OFFSET]
            if mode == OFF:
                t = np.zeros(N, dt)
            elif mode == TORQUE:
                t = u
            elif mode == POSITION:
                d = clamp(u, p[TARGET_LO], p[TARGET_HI]) - q[j]
                pp = p[KP] * d
                v = p[KD] * qd[j]
                t = pp - v
            else:
                d = u - qd[j]
                t = p[KD] * d
            if feed_forward is not None:
                t = t + feed_forward[j]
            out[j] = clamp(t, -p[TORQUE_LIMIT], p[TORQUE_LIMIT])
    assert out.dtype == dt
    return out
