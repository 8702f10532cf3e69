"""TEST INFRASTRUCTURE: NumPy restatement of the policy observation (``jxs_env_observe``), written from the table of the
slot kinds in include/jaxsim_amd.h; it does not import the product.

``observe(block, ...)`` evaluates every slot on a logical ``[rows, N]`` state block.  With ``dtype=None`` the arithmetic runs
in the block's dtype, every operation rounded on its own, in the order the table states: the result is comparable bit for
bit for the kinds made of ``+ - x`` only (``BITWISE_KINDS``; the Inertial and Mixed base velocity).  With
``dtype=np.float64`` it is the truth: the same formulas in float64 on the stored inputs (and the stored offset / scale).
"""

from __future__ import annotations

import numpy as np

STATE_ROW, SOURCE_ROW, BASE_QUAT_UNIT, BASE_ROTATION, BASE_VELOCITY, PROJECTED_GRAVITY = range(6)
INERTIAL, BODY, MIXED = 0, 1, 2
MAX_WIDTH = 4096
COMPONENTS = {BASE_QUAT_UNIT: 4, BASE_ROTATION: 9, BASE_VELOCITY: 6, PROJECTED_GRAVITY: 3}
# error codes of the validity check
OK, BAD_WIDTH, BAD_KIND, BAD_INDEX, BAD_SOURCE = range(5)


def n_rows(n_joints: int, n_points: int) -> int:
    return 13 + 2 * n_joints + 3 * n_points


def tile_block(block: np.ndarray, T: int, pad=0.0) -> np.ndarray:
    """``[rows, N]`` -> the flat storage ``[ceil(N/T)][rows][T]``; the padding columns hold ``pad``."""
    rows, N = block.shape
    nt = -(-N // T)
    wide = np.full((rows, nt * T), pad, dtype=block.dtype)
    wide[:, :N] = block
    return np.ascontiguousarray(wide.reshape(rows, nt, T).transpose(1, 0, 2)).reshape(-1)


def bitwise(kind: int, repr_: int, index: int = 0) -> bool:
    """Is the word of such a slot made of additions, subtractions and multiplications only?"""
    if kind in (STATE_ROW, SOURCE_ROW):
        return True
    return kind == BASE_VELOCITY and repr_ in (INERTIAL, MIXED)


def slot_error(slot, rows: int, source_rows=(0, 0, 0, 0)) -> int:
    kind, source, index = (int(v) for v in slot)
    if kind < 0 or kind > PROJECTED_GRAVITY:
        return BAD_KIND
    if kind == STATE_ROW:
        return OK if 0 <= index < rows else BAD_INDEX
    if kind == SOURCE_ROW:
        if not 0 <= source < 4 or source >= len(source_rows) or source_rows[source] <= 0:
            return BAD_SOURCE
        return OK if 0 <= index < source_rows[source] else BAD_INDEX
    return OK if 0 <= index < COMPONENTS[kind] else BAD_INDEX


def table_error(slots, rows: int, source_rows=(0, 0, 0, 0), D=None) -> tuple[int, int]:
    """``(code, slot)`` of the first refusal of a table, ``(OK, -1)`` for a valid one."""
    D = len(slots) if D is None else D
    if D < 1 or D > MAX_WIDTH:
        return BAD_WIDTH, -1
    for d, slot in enumerate(slots):
        code = slot_error(slot, rows, source_rows)
        if code != OK:
            return code, d
    return OK, -1


def rotation(u):
    """The nine entries (row-major, each ``[N]``) of the rotation matrix of the quaternion rows ``u`` = (w, x, y, z)."""
    w, i, j, l = u
    one, two = u[0].dtype.type(1), u[0].dtype.type(2)
    return [
        one - two * (j * j + l * l), two * (i * j - w * l), two * (i * l + w * j),
        two * (i * j + w * l), one - two * (i * i + l * l), two * (j * l - w * i),
        two * (i * l - w * j), two * (j * l + w * i), one - two * (i * i + j * j),
    ]  # fmt: skip


def cross(p, a):
    return [p[(k + 1) % 3] * a[(k + 2) % 3] - p[(k + 2) % 3] * a[(k + 1) % 3] for k in range(3)]


def derived(block: np.ndarray, n_joints: int, repr_: int) -> dict:
    """kind -> list of component rows ``[N]`` of the four derived kinds, in the dtype of ``block``."""
    n = n_joints
    p, q = list(block[0:3]), list(block[3:7])
    lin, ang = list(block[7 + n : 10 + n]), list(block[10 + n : 13 + n])
    with np.errstate(all="ignore"):
        n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
        nrm = np.sqrt(n2)
        safe = np.where(nrm == 0, nrm.dtype.type(1), nrm)
        u = [np.where(nrm == 0, q[k], q[k] / safe) for k in range(4)]
        R = rotation(u)
        if repr_ == INERTIAL:
            vel = lin + ang
        else:
            pxw = cross(p, ang)
            m = [lin[k] - pxw[k] for k in range(3)]
            if repr_ == MIXED:
                vel = m + ang
            else:  # R^T x: column k of R against x
                vel = [R[k] * x[0] + R[3 + k] * x[1] + R[6 + k] * x[2] for x in (m, ang) for k in range(3)]
        grav = [-R[6 + k] for k in range(3)]
    return {BASE_QUAT_UNIT: u, BASE_ROTATION: R, BASE_VELOCITY: vel, PROJECTED_GRAVITY: grav}


def observe(block: np.ndarray, slots, offset, scale, n_joints: int, repr_: int, sources=(), dtype=None, out_dtype=None) -> np.ndarray:
    """``[N, D]``.  ``block``: ``[rows, N]``; ``sources``: up to four ``[rows_s, N]`` arrays (or ``None``); ``offset`` /
    ``scale``: scalars or ``[D]``, rounded to the block's dtype first (what the table stores)."""
    stored = block.dtype
    dt = np.dtype(dtype or stored)
    slots = np.asarray(slots, dtype=np.int64).reshape(-1, 3)
    D, N = len(slots), block.shape[1]
    off = np.broadcast_to(np.asarray(offset, dtype=stored), (D,)).astype(dt)
    sc = np.broadcast_to(np.asarray(scale, dtype=stored), (D,)).astype(dt)
    blk = block.astype(dt)
    der = derived(blk, n_joints, repr_)
    x = np.empty((D, N), dtype=dt)
    for d, (kind, source, index) in enumerate(slots):
        if kind == STATE_ROW:
            x[d] = blk[index]
        elif kind == SOURCE_ROW:
            x[d] = np.asarray(sources[source])[index].astype(dt)
        else:
            x[d] = der[kind][index]
    with np.errstate(all="ignore"):
        diff = x - off[:, None]
        y = diff * sc[:, None]
    y = np.ascontiguousarray(y.T)
    return y if out_dtype is None else y.astype(out_dtype)


def full_table(rows: int, source_rows=()) -> np.ndarray:
    """Every state row, every row of every source, and every component of the four derived kinds, in that order."""
    slots = [(STATE_ROW, 0, r) for r in range(rows)]
    slots += [(SOURCE_ROW, s, r) for s, rs in enumerate(source_rows) for r in range(rs)]
    slots += [(kind, 0, c) for kind, nc in COMPONENTS.items() for c in range(nc)]
    return np.array(slots, dtype=np.int32)


def bounds(slots, block: np.ndarray, n_joints: int, dtype) -> np.ndarray:
    """``[N, D]`` absolute error bounds of the kinds that are compared with the float64 truth, from the operation count
    (``eps`` of ``dtype``), for offset 0 and scale 1 (an exact slot arithmetic): unit quaternion 4 eps, rotation entries and
    projected gravity 16 eps, base velocity 64 eps (1 + |l| + |p| |w|).  Zero for the state and source rows."""
    eps = float(np.finfo(dtype).eps)
    n = n_joints
    b64 = block.astype(np.float64)
    norm = lambda a: np.sqrt((a * a).sum(axis=0))  # noqa: E731
    vel = 64 * eps * (1 + norm(b64[7 + n : 10 + n]) + norm(b64[0:3]) * norm(b64[10 + n : 13 + n]))
    per_kind = {BASE_QUAT_UNIT: 4 * eps, BASE_ROTATION: 16 * eps, PROJECTED_GRAVITY: 16 * eps}
    slots = np.asarray(slots).reshape(-1, 3)
    out = np.zeros((block.shape[1], len(slots)))
    for d, (kind, _, _) in enumerate(slots):
        out[:, d] = vel if kind == BASE_VELOCITY else per_kind.get(int(kind), 0.0)
    return out
