"""TEST INFRASTRUCTURE: NumPy restatement of the reward and termination flags (``jxs_env_evaluate``), written from the law
in the comment of include/jaxsim_amd.h; it does not import the product.

``evaluate(block, table, ...)`` evaluates every environment of a logical ``[rows, N]`` state block.  With ``dtype=None`` the
arithmetic runs in the block's dtype, every operation rounded on its own, in the order the law states: the result is
comparable bit for bit for terms whose slots are of the ``+ - x`` kinds (``env_observe_ref.bitwise``) and whose outer is the
identity.  With ``dtype=np.float64`` it is the truth: the same formulas in float64 on the stored inputs and the stored
table values.
"""

from __future__ import annotations

import dataclasses

import numpy as np
from env_observe_ref import SOURCE_ROW, STATE_ROW, bitwise, derived, slot_error
from env_observe_ref import OK as SLOT_OK

IDENTITY, ABS, SQUARE, EXCESS = range(4)
OUTER_IDENTITY, OUTER_EXP = range(2)
KIND_TERMINATED, KIND_TRUNCATED = range(2)
TERMINATED, TRUNCATED = 1, 2
MAX_SLOTS, MAX_TERMS, MAX_CONDITIONS = 1024, 32, 32
# error codes of the validity check
OK, BAD_WIDTH, BAD_SLOT, BAD_TARGET, BAD_TERM, BAD_RANGE, BAD_CONDITION, UNOWNED, NOT_FINITE, BAD_LIMITS = range(10)


@dataclasses.dataclass
class Table:
    slots: np.ndarray  # [D, 3]
    offset: np.ndarray  # [D] float64
    scale: np.ndarray  # [D] float64
    targets: np.ndarray  # [D, 2], source -1: none
    terms: np.ndarray  # [K, 4] first, count, inner, outer
    term_params: np.ndarray  # [K, 3] weight, lo, hi
    conds: np.ndarray  # [C, 2] slot, kind
    cond_limits: np.ndarray  # [C, 2] lo, hi
    reward_lo: float = -np.inf
    reward_hi: float = np.inf
    termination_reward: float = 0.0

    @property
    def D(self):
        return len(self.slots)

    @property
    def K(self):
        return len(self.terms)

    @property
    def C(self):
        return len(self.conds)


def make_table(terms=(), conds=(), reward_clip=(-np.inf, np.inf), termination_reward=0.0) -> Table:
    """``terms``: ``dict(slots=[(kind, source, index)], inner=, outer=, weight=, lo=, hi=, offset=, scale=, target=(source, row) or
    per-slot list)``; ``conds``: ``dict(slot=(kind, source, index), kind=, lo=, hi=, offset=, scale=, target=)``.  The slots are
    laid out in the order given, terms first."""
    slots, offset, scale, targets, tinfo, tpar, cinfo, clim = [], [], [], [], [], [], [], []

    def add(mine, spec):
        n = len(mine)
        slots.extend(mine)
        offset.extend(np.broadcast_to(np.asarray(spec.get("offset", 0.0), dtype=np.float64), (n,)))
        scale.extend(np.broadcast_to(np.asarray(spec.get("scale", 1.0), dtype=np.float64), (n,)))
        tg = spec.get("target")
        if tg is None:
            targets.extend([(-1, 0)] * n)
        elif isinstance(tg, tuple):
            targets.extend([tg] * n)
        else:
            assert len(tg) == n
            targets.extend(tg)

    for t in terms:
        tinfo.append((len(slots), len(t["slots"]), t.get("inner", IDENTITY), t.get("outer", OUTER_IDENTITY)))
        tpar.append((t.get("weight", 1.0), t.get("lo", -np.inf), t.get("hi", np.inf)))
        add(list(t["slots"]), t)
    for c in conds:
        cinfo.append((len(slots), c.get("kind", KIND_TERMINATED)))
        clim.append((c.get("lo", -np.inf), c.get("hi", np.inf)))
        add([c["slot"]], c)
    return Table(
        np.array(slots, dtype=np.int32).reshape(-1, 3), np.array(offset, dtype=np.float64), np.array(scale, dtype=np.float64),
        np.array(targets, dtype=np.int32).reshape(-1, 2), np.array(tinfo, dtype=np.int32).reshape(-1, 4),
        np.array(tpar, dtype=np.float64).reshape(-1, 3), np.array(cinfo, dtype=np.int32).reshape(-1, 2),
        np.array(clim, dtype=np.float64).reshape(-1, 2), float(reward_clip[0]), float(reward_clip[1]), float(termination_reward))  # fmt: skip


def _finite_in(v: float, dtype) -> bool:
    with np.errstate(over="ignore"):
        return bool(np.isfinite(v) and np.isfinite(np.float64(v).astype(dtype)))


def _limit_ok(v: float, dtype) -> bool:
    return not np.isnan(v) and (np.isinf(v) or _finite_in(v, dtype))


def table_error(tb: Table, rows: int, source_rows=(0, 0, 0, 0), dtype=np.float32, D=None, K=None, C=None) -> tuple[int, int]:
    """``(code, index)`` of the first refusal of a table, ``(OK, -1)`` for a valid one; the checks in the order of the law's list:
    widths, then per slot (slot, target, offset / scale), per term, per condition, unowned slots, the reward limits."""
    D, K, C = (tb.D if D is None else D), (tb.K if K is None else K), (tb.C if C is None else C)
    if not (1 <= D <= MAX_SLOTS and 0 <= K <= MAX_TERMS and 0 <= C <= MAX_CONDITIONS):
        return BAD_WIDTH, -1
    for d in range(D):
        if slot_error(tb.slots[d], rows, source_rows) != SLOT_OK:
            return BAD_SLOT, d
        s, r = (int(v) for v in tb.targets[d])
        if s != -1 and not (0 <= s < 4 and s < len(source_rows) and source_rows[s] > 0 and 0 <= r < source_rows[s]):
            return BAD_TARGET, d
        if not (_finite_in(tb.offset[d], dtype) and _finite_in(tb.scale[d], dtype)):
            return NOT_FINITE, d
    owned = np.zeros(D, bool)
    for k in range(K):
        first, count, inner, outer = (int(v) for v in tb.terms[k])
        w, lo, hi = tb.term_params[k]
        if not (0 <= inner <= EXCESS and 0 <= outer <= OUTER_EXP):
            return BAD_TERM, k
        if count < 1 or first < 0 or first + count > D or owned[first : first + count].any():
            return BAD_RANGE, k
        owned[first : first + count] = True
        if not _finite_in(w, dtype):
            return NOT_FINITE, k
        if not (lo <= hi and _limit_ok(lo, dtype) and _limit_ok(hi, dtype)):
            return BAD_LIMITS, k
    for c in range(C):
        s, kind = (int(v) for v in tb.conds[c])
        if kind not in (KIND_TERMINATED, KIND_TRUNCATED) or not 0 <= s < D or owned[s]:
            return BAD_CONDITION, c
        owned[s] = True
        lo, hi = tb.cond_limits[c]
        if not (lo <= hi and _limit_ok(lo, dtype) and _limit_ok(hi, dtype)):
            return BAD_LIMITS, c
    if not owned.all():
        return UNOWNED, int(np.argmin(owned))
    if not (tb.reward_lo <= tb.reward_hi and _limit_ok(tb.reward_lo, dtype) and _limit_ok(tb.reward_hi, dtype)):
        return BAD_LIMITS, -1
    if not _finite_in(tb.termination_reward, dtype):
        return NOT_FINITE, -1
    return OK, -1


def _clamp(x, lo, hi):
    """x < lo ? lo : (hi < x ? hi : x), element-wise: a NaN stays."""
    return np.where(x < lo, lo, np.where(hi < x, hi, x)).astype(x.dtype)


def slot_words(block: np.ndarray, tb: Table, n_joints: int, repr_: int, sources=(), dtype=None) -> np.ndarray:
    """``y`` ``[D, N]``: the word of every slot."""
    stored = block.dtype
    dt = np.dtype(dtype or stored)
    D, N = tb.D, block.shape[1]
    off, sc = tb.offset.astype(stored).astype(dt), tb.scale.astype(stored).astype(dt)
    blk = block.astype(dt)
    der = derived(blk, n_joints, repr_)
    y = np.empty((D, N), dtype=dt)
    with np.errstate(all="ignore"):
        for d, (kind, source, index) in enumerate(tb.slots):
            if kind == STATE_ROW:
                x = blk[index]
            elif kind == SOURCE_ROW:
                x = np.asarray(sources[source])[index].astype(dt)
            else:
                x = der[int(kind)][index]
            ts, tr = tb.targets[d]
            if ts >= 0:
                x = x - np.asarray(sources[ts])[tr].astype(dt)
            diff = x - off[d]
            y[d] = diff * sc[d]
    return y


def evaluate(block: np.ndarray, tb: Table, n_joints: int, repr_: int, sources=(), steps=None, max_steps=0, dtype=None) -> dict:
    """``dict(reward [N], done [N] uint8, fired [N] uint32, terms [N, K], steps [N] int32 or None, y [D, N])``."""
    stored = block.dtype
    dt = np.dtype(dtype or stored)
    N, K, C = block.shape[1], tb.K, tb.C
    y = slot_words(block, tb, n_joints, repr_, sources, dtype)
    par = tb.term_params.astype(stored).astype(dt)
    lim = tb.cond_limits.astype(stored).astype(dt)
    one, zero = dt.type(1), dt.type(0)
    p = np.zeros((K, N), dtype=dt)
    with np.errstate(all="ignore"):
        for t, (first, count, inner, outer) in enumerate(tb.terms):
            s = None
            for d in range(first, first + count):
                if inner == ABS:
                    v = np.abs(y[d])
                elif inner == SQUARE:
                    v = y[d] * y[d]
                elif inner == EXCESS:
                    v = np.maximum(np.abs(y[d]) - one, zero)  # (np.maximum hands a NaN on)
                else:
                    v = y[d]
                s = v if s is None else s + v
            o = np.exp(-s) if outer == OUTER_EXP else s
            p[t] = _clamp((par[t, 0] * o).astype(dt), par[t, 1], par[t, 2])
        r = np.zeros(N, dtype=dt)
        for t in range(K):
            r = p[t].copy() if t == 0 else r + p[t]
        r = _clamp(r, np.asarray(tb.reward_lo, stored).astype(dt), np.asarray(tb.reward_hi, stored).astype(dt))
        done = np.zeros(N, np.uint8)
        fired = np.zeros(N, np.uint32)
        for c, (slot, kind) in enumerate(tb.conds):
            f = ~((lim[c, 0] <= y[slot]) & (y[slot] <= lim[c, 1]))
            fired |= np.where(f, np.uint32(1 << c), np.uint32(0)).astype(np.uint32)
            done |= np.where(f, np.uint8(1 << int(kind)), np.uint8(0)).astype(np.uint8)
        new_steps = None
        if steps is not None:
            n = np.asarray(steps, np.int32) + np.int32(1)
            done |= np.where(n >= max_steps, np.uint8(TRUNCATED), np.uint8(0)).astype(np.uint8)
            new_steps = np.where(done != 0, np.int32(0), n).astype(np.int32)
        r = np.where((done & TERMINATED) != 0, r + np.asarray(tb.termination_reward, stored).astype(dt), r).astype(dt)
    return dict(reward=r, done=done, fired=fired, terms=np.ascontiguousarray(p.T), steps=new_steps, y=y)


def slot_bitwise(tb: Table, repr_: int) -> np.ndarray:
    """``[D]`` bool: is the word of the slot made of ``+ - x`` only?"""
    return np.array([bitwise(int(k), repr_) for k, _, _ in tb.slots], dtype=bool)


def term_classes(tb: Table, repr_: int):
    """``(exact, exp, derived)`` bool ``[K]``: terms compared bit for bit, ``EXP`` terms on bitwise slots, terms on derived kinds."""
    sb = slot_bitwise(tb, repr_)
    on_bitwise = np.array([sb[f : f + n].all() for f, n, _, _ in tb.terms], dtype=bool).reshape(-1)
    is_exp = (tb.terms[:, 3] == OUTER_EXP) if tb.K else np.zeros(0, bool)
    return on_bitwise & ~is_exp, on_bitwise & is_exp, ~on_bitwise


def truth(block, tb, n_joints, repr_, sources=(), steps=None, max_steps=0) -> dict:
    return evaluate(block, tb, n_joints, repr_, sources, steps, max_steps, dtype=np.float64)


def slot_bounds(block: np.ndarray, tb: Table, n_joints: int, repr_: int, sources=()) -> np.ndarray:
    """``[D, N]`` absolute error bound of every slot's word ``y`` against the float64 truth, in the block's dtype.  The raw
    value of a derived kind errs by ``env_observe_ref.bounds`` (unit quaternion 4 eps, rotation and gravity 16 eps, velocity
    64 eps (1 + |l| + |p||w|)); a state or source row is exact.  The target difference and the offset difference add one
    rounding each, the scale one more: ``|dy| <= (b_raw + eps |x| + eps |x - off|) |scale| + eps |y|``, evaluated on the truth
    with a factor 2 for the second-order terms."""
    from env_observe_ref import bounds as raw_bounds

    eps = float(np.finfo(block.dtype).eps)
    b_raw = raw_bounds(tb.slots, block, n_joints, block.dtype).T  # [D, N]
    one = dataclasses.replace(tb, offset=np.zeros(tb.D), scale=np.ones(tb.D))
    x = np.abs(slot_words(block, one, n_joints, repr_, sources, dtype=np.float64))
    off = tb.offset.astype(block.dtype).astype(np.float64)[:, None]
    sc = np.abs(tb.scale.astype(block.dtype).astype(np.float64))[:, None]
    y = np.abs(slot_words(block, tb, n_joints, repr_, sources, dtype=np.float64))
    has_target = (tb.targets[:, 0] >= 0)[:, None]
    return 2 * ((b_raw + eps * x * has_target + eps * np.abs(x - off)) * sc + eps * y)


def bounds(block: np.ndarray, tb: Table, n_joints: int, repr_: int, sources=()) -> np.ndarray:
    """``[N, K]`` absolute error bound of every term's contribution against the float64 truth.  With ``b_d`` the bound of a
    slot's word: the inner value errs by ``b`` (identity, abs, excess: 1-Lipschitz, excess with one more rounding) or
    ``2 |y| b + b^2 + eps y^2`` (square); the sequential sum of ``n`` values adds ``(n - 1) eps sum |v|``; ``exp(-s)`` errs
    by ``exp(-s) (e^{ds} - 1) + 2 eps exp(-s)``; the weight adds one rounding; the clamp is 1-Lipschitz.  A factor 2 covers
    second-order terms."""
    eps = float(np.finfo(block.dtype).eps)
    tr = truth(block, tb, n_joints, repr_, sources)
    y, b = np.abs(tr["y"]), slot_bounds(block, tb, n_joints, repr_, sources)
    N = block.shape[1]
    out = np.zeros((N, tb.K))
    par = tb.term_params.astype(block.dtype).astype(np.float64)
    with np.errstate(all="ignore"):
        for t, (first, count, inner, outer) in enumerate(tb.terms):
            ds, sabs, s = np.zeros(N), np.zeros(N), np.zeros(N)
            for d in range(first, first + count):
                if inner == SQUARE:
                    v, dv = y[d] * y[d], 2 * y[d] * b[d] + b[d] * b[d] + eps * y[d] * y[d]
                elif inner == EXCESS:
                    v = np.maximum(y[d] - 1, 0)
                    dv = b[d] + eps * (y[d] + 1)
                else:
                    v, dv = y[d], b[d]
                ds, sabs = ds + dv, sabs + v
                s = s + (tr["y"][d] if inner == IDENTITY else v)
            ds = ds + (count - 1) * eps * sabs
            if outer == OUTER_EXP:
                o = np.exp(-s)
                do = o * np.expm1(ds) + 2 * eps * o
            else:
                o, do = np.abs(s), ds
            out[:, t] = 2 * (np.abs(par[t, 0]) * do + eps * np.abs(par[t, 0] * o))
    return out
