"""TEST INFRASTRUCTURE: what the CPU tests of the per-environment operations (tests/test_env_*_cpu.py) share with one
another and with their GPU twins -- the ``lib`` fixture and the refusal check of the C ABI, stand-ins for foreign arrays
and device data, bitwise comparisons, and per family the case builders and the check of an implementation (host harness or
device) against its NumPy restatement.  The counterpart of tests/env_gpu_support.py; no test lives here."""

import types

import numpy as np
import pytest

import env_act_ref as act_ref
import env_evaluate_ref as eva
import env_observe_ref as obs
import env_ops_ref as ops
import env_random_ref as rnd
from jaxsim_amd import _lib
from jaxsim_amd.data import JaxSimModelData
from jaxsim_amd.model import VelRepr


# ---- every family: the C ABI without a device, foreign arrays, words -----------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def refused(lib, rc, *words):
    assert rc == -1
    msg = lib.jxs_last_error().decode()
    assert msg and any(w in msg for w in words), msg


class Foreign:
    """What another framework hands over: a ``__cuda_array_interface__`` over memory this library does not own."""

    def __init__(self, shape, typestr, ptr=0x1000, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}


def stub_data(model, N, dtype, tile=2):
    """A data object around a state that is no device buffer: every refusal below must come before the first device call."""
    from jaxsim_amd.state import StateLayout

    state = types.SimpleNamespace(rows=StateLayout.of(model).n_rows, cols=N, tile=tile, dtype=np.dtype(dtype), ptr=None)
    return JaxSimModelData(model, state, VelRepr.Mixed, True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    differ = bits(got) != bits(want)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} words differ, first at {int(np.argmax(differ))}"


def same_words(got, want, what=""):
    """Bit for bit; two NaNs are the same word (the module's docstring)."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    differ = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} words differ, first at {int(np.argmax(differ))}: {got[differ][:3]} != {want[differ][:3]}"


# ---- observe (tests/env_observe_ref.py) ----------------------------------------------------------------------------
REPRS = (obs.INERTIAL, obs.BODY, obs.MIXED)
SOURCE_ROWS = (5, 0, 3)  # sources 0 and 2; source 1 does not exist


def observe_batch_sizes(T):
    return sorted({1, T, 2 * T + 1})


def special_envs(n, N):
    """(environment with a zero quaternion, environment with a NaN joint row) -- None where the batch is too small."""
    return (N - 1 if N >= 2 else None), (N // 2 - 1 if N >= 3 and n > 0 else None)


def make_block(n, n_points, N, dtype, seed):
    """A state block ``[rows, N]``: |p| <= 2, velocities <= 5, quaternions 1e-3 off unit norm; one environment with a zero
    quaternion and one with a NaN joint-position row where the batch has room for them."""
    rng = np.random.default_rng(seed)
    rows = obs.n_rows(n, n_points)
    blk = rng.uniform(-1.0, 1.0, size=(rows, N))
    p = rng.normal(size=(3, N))
    blk[0:3] = p / np.linalg.norm(p, axis=0) * rng.uniform(0.0, 2.0, size=N)
    q = rng.normal(size=(4, N))
    blk[3:7] = q / np.linalg.norm(q, axis=0) * (1.0 + 1e-3 * rng.choice([-1.0, 1.0], size=N))
    blk[7 + n : 13 + n] = rng.uniform(-5.0, 5.0, size=(6, N))
    blk[13 + n : 13 + 2 * n] = rng.uniform(-5.0, 5.0, size=(n, N))
    zero_q, nan_env = special_envs(n, N)
    if zero_q is not None:
        blk[3:7, zero_q] = 0.0
    if nan_env is not None:
        blk[7 + n // 2, nan_env] = np.nan
    return blk.astype(dtype)


def make_sources(N, dtype, seed):
    rng = np.random.default_rng(seed + 1)
    return [None if r == 0 else rng.uniform(-3.0, 3.0, size=(r, N)).astype(dtype) for r in SOURCE_ROWS]


def tiled_sources(srcs, T):
    """The sources as the harness and the kernel take them; the padding columns hold NaN."""
    return [None if s is None else (obs.tile_block(s, T, pad=np.nan), s.shape[0]) for s in srcs]


def same_or_both_nan(got, want, mask, what):
    """Bit for bit where ``mask`` holds, a NaN comparing equal to any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    same = (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
    bad = ~same & mask
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {tuple(np.argwhere(bad)[0])}"


def check_observe_against_the_restatement(observe, n, n_points, T, dtype, what, seed=0):
    """``observe(storage, slots, offset, scale, N, repr, sources, out_ld, out_dtype)`` -> ``[N, out_ld]`` (untouched words NaN)
    against tests/env_observe_ref.py over the batch sizes and the three representations.  Returns the worst ratio of an
    error to its bound per kind."""
    rows = obs.n_rows(n, n_points)
    slots = obs.full_table(rows, SOURCE_ROWS)
    D = len(slots)
    rng = np.random.default_rng(rows + T)
    offsets, scales = rng.uniform(-2.0, 2.0, size=D).astype(dtype), rng.uniform(0.25, 4.0, size=D).astype(dtype)
    worst = {}
    for N in observe_batch_sizes(T):
        blk = make_block(n, n_points, N, dtype, seed=seed + 100 * N + rows)
        srcs = make_sources(N, dtype, seed=N)
        storage, tsrcs = obs.tile_block(blk, T, pad=np.nan), tiled_sources(srcs, T)
        for repr_ in REPRS:
            tag = f"{what} N={N} repr={repr_}"
            exact = np.array([obs.bitwise(k, repr_) for k, _, _ in slots])
            cols = np.broadcast_to(exact[None, :], (N, D))
            # the + - x kinds, bit for bit: as they are, and with an offset and a scale; into a wider row too
            for off, sc in ((0.0, 1.0), (offsets, scales)):
                want = obs.observe(blk, slots, off, sc, n, repr_, srcs)
                got = observe(storage, slots, off, sc, N, repr_, tsrcs, D, dtype)
                same_or_both_nan(got, want, cols, tag)
            wide = observe(storage, slots, offsets, scales, N, repr_, tsrcs, D + 3, dtype)
            assert np.isnan(wide[:, D:]).all(), f"{tag}: the gap columns of a wider row were written"
            same_or_both_nan(np.ascontiguousarray(wide[:, :D]), want, cols, f"{tag} out_ld=D+3")
            if dtype == np.float64:  # rounded once, at the store
                got32 = observe(storage, slots, offsets, scales, N, repr_, tsrcs, D, np.float32)
                same_or_both_nan(got32, want.astype(np.float32), cols, f"{tag} out_dtype=float32")
            # the other kinds against the float64 truth on the stored inputs (offset 0, scale 1: the slot adds no rounding)
            got = observe(storage, slots, 0.0, 1.0, N, repr_, tsrcs, D, dtype)
            truth = obs.observe(blk, slots, 0.0, 1.0, n, repr_, srcs, dtype=np.float64)
            bound = obs.bounds(slots, blk, n, dtype)
            err = np.abs(got.astype(np.float64) - truth)
            for kind in obs.COMPONENTS:
                sel = (slots[:, 0] == kind) & ~exact
                if not sel.any():
                    continue
                assert np.isfinite(got[:, sel]).all(), f"{tag}: a derived value of kind {kind} is not finite"
                ratio = float((err[:, sel] / bound[:, sel]).max())
                worst[kind] = max(worst.get(kind, 0.0), ratio)
                assert ratio <= 1.0, f"{tag}: kind {kind} misses its bound by a factor of {ratio:.3g}"
    return worst


# ---- evaluate (tests/env_evaluate_ref.py; state blocks and sources as for observe) ---------------------------------
S, SRC, VEL, GRAV, ROT, QUAT = obs.STATE_ROW, obs.SOURCE_ROW, obs.BASE_VELOCITY, obs.PROJECTED_GRAVITY, obs.BASE_ROTATION, obs.BASE_QUAT_UNIT


def ragged_batch_sizes(T):
    return sorted({1, T - 1, T + 1, 9 * T + 1} - {0})


def term_list(n, seed):
    """Every inner, both outers, targets, finite and infinite clips, a one-slot term and an n-slot term (23 for the humanoid)."""
    rng = np.random.default_rng(seed)
    q, qd = [(S, 0, 7 + j) for j in range(n)], [(S, 0, 13 + n + j) for j in range(n)]
    terms = [
        dict(slots=q, inner=eva.EXCESS, offset=rng.uniform(-0.3, 0.3, n), scale=rng.uniform(1.5, 3.0, n), weight=-2.0),
        dict(slots=qd, inner=eva.SQUARE, weight=-0.01, lo=-0.5),
        dict(slots=[(S, 0, 2)], offset=0.5, weight=1.5),
        dict(slots=[(SRC, 0, k) for k in range(3)], inner=eva.ABS, target=[(2, k) for k in range(3)], hi=2.0, weight=0.7),
        dict(slots=[(VEL, 0, k) for k in range(3)], inner=eva.SQUARE, outer=eva.OUTER_EXP, target=[(0, k) for k in range(3)], scale=0.5),
        dict(slots=qd[:2], inner=eva.SQUARE, outer=eva.OUTER_EXP, scale=0.3, weight=0.5, offset=0.1),
        dict(slots=[(GRAV, 0, 0), (GRAV, 0, 1)], inner=eva.SQUARE, weight=-1.0),
        dict(slots=[(ROT, 0, 8)], weight=0.25, lo=-0.1, hi=0.2),
        dict(slots=[(QUAT, 0, 0)], inner=eva.ABS, scale=2.0),
        dict(slots=[(VEL, 0, k) for k in range(3, 6)], inner=eva.ABS, lo=-1.0, hi=1.0, weight=0.1),
        dict(slots=[(SRC, 2, 1), (S, 0, 0)], inner=eva.IDENTITY, outer=eva.OUTER_EXP, scale=0.2, weight=-0.3),
    ]
    return [t for t in terms if len(t["slots"])]  # (a model without joints has no joint terms)


def gap_threshold(values, bound):
    """A threshold in the widest gap of the finite ``values``, and the distance from it to the nearest of them over ``bound``."""
    v = np.sort(values[np.isfinite(values)])
    if len(v) < 2:
        return (float(v[0]) + 1.0 if len(v) else 0.0), np.inf
    k = int(np.argmax(np.diff(v)))
    return float((v[k] + v[k + 1]) / 2), float((v[k + 1] - v[k]) / 2 / max(bound, 1e-300))


def cond_list(n, blk, srcs, repr_):
    """Windows on exact kinds, and thresholds on derived kinds placed in the widest gap of the batch's float64 values."""
    conds = [
        dict(slot=(S, 0, 2), lo=-0.5, hi=0.8),
        dict(slot=(SRC, 2, 1), hi=2.0, kind=eva.KIND_TRUNCATED),
        dict(slot=(S, 0, 7 if n else 1), offset=0.1, scale=1.7, lo=-1.0, hi=1.0),
        dict(slot=(SRC, 0, 4), target=(2, 0), lo=-2.5, kind=eva.KIND_TRUNCATED),
    ]
    probe = eva.make_table(conds=[dict(slot=(GRAV, 0, 2)), dict(slot=(VEL, 0, 0), scale=0.5), dict(slot=(ROT, 0, 0), offset=0.25)])
    y = eva.slot_words(blk, probe, n, repr_, srcs, dtype=np.float64)
    b = eva.slot_bounds(blk, probe, n, repr_, srcs)
    margins = []
    for k, (slot, extra) in enumerate((((GRAV, 0, 2), {}), ((VEL, 0, 0), dict(scale=0.5)), ((ROT, 0, 0), dict(offset=0.25)))):
        th, margin = gap_threshold(y[k], float(b[k][np.isfinite(b[k])].max(initial=0.0)))
        margins.append(margin)
        conds.append(dict(slot=slot, **extra, **({"hi": th} if k != 1 else {"lo": th}), kind=eva.KIND_TRUNCATED if k == 2 else eva.KIND_TERMINATED))
    return conds, margins


def check_evaluate_against_the_restatement(evaluate, n, n_points, T, dtype, what, sizes=None, seed=0):
    """``evaluate(storage, table, rows, n, N, T, repr, tiled sources, steps=, max_steps=, fill=)`` -> dict of outputs against
    tests/env_evaluate_ref.py over the batch sizes and the three representations.  Returns the worst ratios."""
    rows = obs.n_rows(n, n_points)
    eps = float(np.finfo(dtype).eps)
    worst = {"exp": 0.0, "derived": 0.0, "reward": 0.0}
    for N in sizes or ragged_batch_sizes(T):
        blk = make_block(n, n_points, N, dtype, seed=seed + 100 * N + rows)
        srcs = make_sources(N, dtype, seed=N)
        storage, tsrcs = obs.tile_block(blk, T, pad=np.nan), tiled_sources(srcs, T)
        steps = np.random.default_rng(N).integers(0, 9, size=N).astype(np.int32)
        for repr_ in REPRS:
            tag = f"{what} N={N} repr={repr_}"
            terms = term_list(n, seed=rows)
            conds, margins = cond_list(n, blk, srcs, repr_)
            # (the thresholds on derived kinds are clear of every environment's value by more than its bound: asserted for all)
            assert min(margins) > 1.0, f"{tag}: a derived threshold lies within the bound of some environment: {margins}"
            tb = eva.make_table(terms, conds, reward_clip=(-3.0, 2.5), termination_reward=-1.25)
            exact, is_exp, is_derived = eva.term_classes(tb, repr_)
            want = eva.evaluate(blk, tb, n, repr_, srcs, steps=steps, max_steps=7)
            got = evaluate(storage, tb, rows, n, N, T, repr_, tsrcs, steps=steps, max_steps=7)
            for k in ("done", "fired", "steps"):
                assert np.array_equal(got[k], want[k]), f"{tag}: {k} {got[k]} != {want[k]}"
            same_or_both_nan(got["terms"], want["terms"], np.broadcast_to(exact[None, :], (N, tb.K)), f"{tag} terms")
            truth = eva.truth(blk, tb, n, repr_, srcs, steps=steps, max_steps=7)
            assert np.array_equal(np.isnan(got["terms"]), np.isnan(truth["terms"])), f"{tag}: NaN terms"
            with np.errstate(invalid="ignore"):
                err = np.abs(got["terms"].astype(np.float64) - want["terms"].astype(np.float64))
                rel = err / (4 * eps * np.abs(want["terms"].astype(np.float64)))
                terr = np.abs(got["terms"].astype(np.float64) - truth["terms"]) / eva.bounds(blk, tb, n, repr_, srcs)
            if is_exp.any():
                r = float(np.nanmax(np.where(err[:, is_exp] == 0, 0.0, rel[:, is_exp])))
                worst["exp"] = max(worst["exp"], r)
                assert r <= 1.0, f"{tag}: an EXP term misses 4 eps |want| by a factor of {r:.3g}"
            if is_derived.any():
                r = float(np.nanmax(terr[:, is_derived]))
                worst["derived"] = max(worst["derived"], r)
                assert r <= 1.0, f"{tag}: a term on a derived kind misses its bound by a factor of {r:.3g}"
            # the reward of the whole table: within the terms' bounds and the K roundings of the sum
            tp = np.abs(truth["terms"])
            rb = eva.bounds(blk, tb, n, repr_, srcs).sum(axis=1) + 2 * (tb.K + 1) * eps * (tp.sum(axis=1) + abs(tb.termination_reward))
            with np.errstate(invalid="ignore"):
                r = float(np.nanmax(np.abs(got["reward"].astype(np.float64) - truth["reward"]) / rb))
            assert np.array_equal(np.isnan(got["reward"]), np.isnan(truth["reward"])), f"{tag}: NaN rewards"
            worst["reward"] = max(worst["reward"], r)
            assert r <= 1.0, f"{tag}: the reward misses its bound by a factor of {r:.3g}"
            # the bit-exact terms alone: reward, terms, done, fired and steps bit for bit; into a wider terms row too
            xt = eva.make_table([t for t, e in zip(terms, exact) if e], conds, reward_clip=(-3.0, 2.5), termination_reward=-1.25)
            want = eva.evaluate(blk, xt, n, repr_, srcs, steps=steps, max_steps=7)
            got = evaluate(storage, xt, rows, n, N, T, repr_, tsrcs, steps=steps, max_steps=7, terms_ld=xt.K + 3, fill=np.nan)
            all_ = np.ones((N, xt.K), bool)
            same_or_both_nan(got["reward"], want["reward"], all_[:, 0], f"{tag} exact reward")
            same_or_both_nan(np.ascontiguousarray(got["terms"][:, : xt.K]), want["terms"], all_, f"{tag} exact terms")
            assert np.isnan(got["terms"][:, xt.K :]).all(), f"{tag}: the gap columns of a wider terms row were written"
            for k in ("done", "fired", "steps"):
                assert np.array_equal(got[k], want[k]), f"{tag}: exact {k}"
    return worst


# ---- act (tests/env_act_ref.py) ------------------------------------------------------------------------------------
SPECIAL = (np.nan, np.inf, -np.inf, -0.0)  # the action words of environments 0 .. 3 of a batch of at least five


def make_action_table(n, A, seed):
    """A table over n joints and an action tensor of A columns: the four modes in turn, every fifth joint without a column,
    infinite and finite clips, target windows and torque limits, a clip of zero, an offset of -0; the columns in a shuffled
    order, and at least one column of a wide enough tensor left unnamed."""
    rng = np.random.default_rng(1000 + seed)
    free = list(rng.permutation(A)[: max(A - 1, 1) if A > 1 else A])
    joints, params = np.zeros((n, 2), np.int32), np.zeros((n, 8))
    for j in range(n):
        column = -1 if (j % 5 == 4 or not free) else int(free.pop())
        joints[j] = ((j + 2) % 4 if n >= 4 else (act_ref.POSITION, act_ref.VELOCITY, act_ref.TORQUE, act_ref.OFF)[(j + seed) % 4], column)
        lo, hi = [(-np.inf, np.inf), (rng.uniform(-0.6, -0.1), rng.uniform(0.1, 0.6)), (-np.inf, rng.uniform(0.1, 0.6)), (rng.uniform(-0.6, -0.1), np.inf)][j % 4 if j % 8 < 4 else (j + 1) % 4]
        params[j] = [rng.uniform(0.25, 2.0) * (-1 if j % 6 == 5 else 1), rng.uniform(-0.5, 0.5), rng.uniform(5, 50), rng.uniform(0.1, 2.0),
                     np.inf if j % 3 == 0 else rng.uniform(0.3, 1.0), lo, hi, np.inf if j % 7 < 2 else rng.uniform(2, 20)]  # fmt: skip
    if n >= 12:
        params[1, act_ref.OFFSET] = -0.0  # (joint 1 is a torque joint: an action of -0 stays -0)
        params[1, act_ref.SCALE] = 1.0
        params[6, act_ref.ACTION_CLIP] = 0.0  # clamp(x, -0, 0)
    return joints, params


def make_case(n, n_points, N, dtype, act_dtype, seed, gap=3):
    """``(block [rows, N], joints, params, actions [N, A + gap], A, feed_forward [n, N])``: NaN in every state row that is
    neither a joint position nor a joint velocity, in the gap columns and in the columns the table does not name; the action
    rows 0 .. 3 of a batch of five or more are all NaN, +inf, -inf and -0."""
    rng = np.random.default_rng(seed)
    rows = act_ref.n_rows(n, n_points)
    A = n + 2
    joints, params = make_action_table(n, A, seed)
    blk = np.full((rows, N), np.nan, dtype)
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)  # noqa: E731
    blk[act_ref.row_q(n) : act_ref.row_q(n) + n] = (rng.uniform(0.05, 1.5, (n, N)) * sign((n, N))).astype(dtype)
    blk[act_ref.row_qd(n) : act_ref.row_qd(n) + n] = (rng.uniform(0.05, 4.0, (n, N)) * sign((n, N))).astype(dtype)
    actions = np.full((N, A + gap), np.nan, act_dtype)
    named = joints[joints[:, 1] >= 0, 1]
    actions[:, named] = (rng.uniform(0.02, 2.5, (N, len(named))) * sign((N, len(named)))).astype(act_dtype)
    if N >= 5:
        for e, v in enumerate(SPECIAL):
            actions[e, named] = v
    ff = (rng.uniform(0.1, 3.0, (n, N)) * sign((n, N))).astype(dtype)
    return blk, joints, params, actions, A, ff


def check_act_against_the_restatement(act, n, n_points, T, dtype, what, seed=0, sizes=None):
    """``act(storage, joints, params, actions, A, N, ff_storage or None) -> flat tiled torque block``, held against the
    restatement over the batch sizes, float32 and same-dtype actions, with and without feed-forward.  The padding columns
    of the state and of the feed-forward block hold NaN; those of the result must be +0."""
    rows = act_ref.n_rows(n, n_points)
    for N in sizes or ragged_batch_sizes(T):
        for act_dtype in {np.dtype(np.float32), np.dtype(dtype)}:
            blk, joints, params, actions, A, ff = make_case(n, n_points, N, dtype, act_dtype, seed + 7 * N)
            storage = act_ref.tile_block(blk, T, pad=np.nan)
            q, qd = blk[act_ref.row_q(n) : act_ref.row_q(n) + n], blk[act_ref.row_qd(n) : act_ref.row_qd(n) + n]
            for with_ff in (False, True):
                tag = f"{what} N={N} actions {act_dtype.name} ff={with_ff}"
                got = act(storage, joints, params, actions, A, N, act_ref.tile_block(ff, T, pad=np.nan) if with_ff else None)
                tau, pad = act_ref.untile_block(got, n, N, T)
                assert (bits(pad) == 0).all(), f"{tag}: the padding columns of the torque block are not +0"
                want = act_ref.act(q, qd, joints, params, actions, ff if with_ff else None)
                same_words(tau, want, tag)
                special = N >= 5 and (joints[:, 1] >= 0).any()
                assert np.isfinite(tau[:, len(SPECIAL) if N >= 5 else 0 :]).all(), f"{tag}: a NaN from a gap, an unnamed column or a padding column"
                if special:
                    driven = joints[:, 1] >= 0
                    assert np.isnan(tau[driven & (joints[:, 0] != act_ref.OFF), 0]).all(), f"{tag}: a NaN action must pass through"
                    assert not np.isnan(tau[~driven, 0]).any()


# ---- randomize (tests/env_random_ref.py) ---------------------------------------------------------------------------
def named_words(rows, N, T, take):
    """For every flat word of the storage: does it belong to an environment the mask names?"""
    env = ops.word_env(rows, N, T)
    out = np.zeros(env.shape, dtype=bool)
    real = env < N
    out[real] = take[env[real]]
    return out


def check_contract(got, before, mask, n, n_points, N, T, bounds, seed, draw, first_env, floating, repr_, what=""):
    """The contract of jxs_env_randomize on a tiled storage ``got`` that held ``before``."""
    dt = before.dtype
    u, eps = ops.bits_dtype(dt), float(np.finfo(dt).eps)
    L = rnd.Rows(n, n_points)
    with np.errstate(all="ignore"):  # (the environments that keep their random bits hold NaNs and infinities)
        want, exact, take = rnd.randomize(before, mask, n, n_points, N, T, bounds, seed, draw, first_env, floating, repr_)
    named = named_words(L.rows, N, T, take)
    assert (got.view(u)[~named] == before.view(u)[~named]).all(), f"{what}: words of unnamed environments or of padding columns changed"
    tk = np.nonzero(take)[0]
    if tk.size == 0:
        return
    g = rnd.untile(got, L.rows, N, T)[:, tk]
    w = rnd.untile(want, L.rows, N, T)[:, tk]
    bw = L.bitwise(floating, repr_)
    differ = g.view(u)[bw] != w.view(u)[bw]
    assert not differ.any(), f"{what}: {int(differ.sum())} words of the uniform / zero rows differ"
    assert np.isfinite(g).all(), what
    dq = np.abs(g[L.quat : L.quat + 4].astype(np.float64) - exact[L.quat : L.quat + 4, tk]).max()
    assert dq <= 16 * eps, f"{what}: quaternion off by {dq / eps:.1f} eps"
    if floating and repr_ != rnd.INERTIAL:
        x = rnd.variables(bounds, first_env + tk, seed, draw)
        lin, ang = x[6 + n : 9 + n], x[9 + n : 12 + n]
        v = rnd.velocity_of_block(L, g, lin, ang, repr_)
        scale = np.maximum(1.0, np.linalg.norm(lin, axis=0) + np.linalg.norm(g[0:3].astype(np.float64), axis=0) * np.linalg.norm(ang, axis=0))
        dv = (np.abs(g[L.vlin : L.vlin + 6].astype(np.float64) - v) / scale).max()
        assert dv <= 32 * eps, f"{what}: base velocity off by {dv / eps:.1f} eps (scaled)"
    if not floating:
        assert (g.view(u)[L.vlin : L.vlin + 6] == 0).all(), f"{what}: a fixed base must get six exact zeros"
