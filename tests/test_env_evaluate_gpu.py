"""The reward and the termination flags on the device: jxs_env_evaluate on guarded raw buffers against the checks the host
harness is held to (tests/test_env_evaluate_cpu.py) and against the harness itself; state and sources inside NaN
surroundings; the Python layer (``js.data.RewardSpec`` / ``JaxSimModelData.evaluate``) against the host properties of the same
data object; the loop step -> evaluate -> reset_random_where(done) -> observe against the same loop through the host;
refusals."""

import ctypes as C

import numpy as np
import pytest

import env_evaluate_emul as emul
import env_evaluate_ref as ref
import env_observe_ref as oref
import helpers
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from env_cpu_support import check_evaluate_against_the_restatement, cond_list, make_block, make_sources, same_or_both_nan, SOURCE_ROWS, term_list, tiled_sources
from env_gpu_support import CONTACT, DTYPES, MODELS, Guarded, InNaN, assert_same_bits, icub_data, same_words
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceArray, DeviceIndices, DeviceMask, DeviceMatrix, DeviceWords
from jaxsim_amd.state import StateLayout

pytestmark = pytest.mark.gpu

S = oref.STATE_ROW


class Table:
    """A ``jxs_evaluation`` of a device model from an ``env_evaluate_ref.Table``, destroyed with the object."""

    def __init__(self, dm, tb, source_rows=SOURCE_ROWS):
        d, self.keep = emul.desc(tb)
        desc = _lib.EvaluationDesc()
        desc.D, desc.K, desc.C = d.D, d.K, d.C
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        cast = lambda a, t: C.cast(C.c_void_p(a.ctypes.data if a.size else None), t)  # noqa: E731
        k = self.keep
        desc.slots, desc.targets, desc.offset, desc.scale = cast(k[0], i32), cast(k[1], i32), cast(k[2], f64), cast(k[3], f64)
        desc.terms, desc.term_params, desc.conditions, desc.condition_limits = cast(k[4], i32), cast(k[5], f64), cast(k[6], i32), cast(k[7], f64)
        desc.reward_lo, desc.reward_hi, desc.termination_reward = tb.reward_lo, tb.reward_hi, tb.termination_reward
        desc.source_rows = (C.c_int32 * 4)(*(list(source_rows) + [0] * (4 - len(source_rows))))
        self.handle, self.K = C.c_void_p(), tb.K
        self.rc = _lib.load().jxs_evaluation_create(dm.handle, C.byref(desc), C.byref(self.handle))

    def __del__(self):
        if self.handle.value:
            _lib.load().jxs_evaluation_destroy(self.handle)


def env_evaluate(dm, table, state_ptr, source_ptrs, N, repr_, reward=None, reward_dtype=np.float32, done=None, fired=None, terms=None,
                 terms_dtype=np.float32, terms_ld=0, steps=None, max_steps=0):  # fmt: skip
    ptrs = (C.c_void_p * 4)(*(list(source_ptrs) + [None] * (4 - len(source_ptrs))))
    vp = lambda p: None if p is None else C.c_void_p(p)  # noqa: E731
    return _lib.load().jxs_env_evaluate(dm.handle, table.handle, C.c_void_p(state_ptr), ptrs, N, repr_, vp(reward), _lib.dtype_code(reward_dtype), vp(done),
                                        vp(fired), vp(terms), _lib.dtype_code(terms_dtype), terms_ld, vp(steps), max_steps, runtime._sp())  # fmt: skip


def pattern_of(count, dtype):
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    return np.full(count, 0x5A5A5A5A5A5A5A5A & np.iinfo(u).max, dtype=u).view(dtype)


def device_evaluate(dm):
    """The ``evaluate`` of tests/test_env_evaluate_cpu.py::check_evaluate_against_the_restatement on the device.  Every output lies in a
    guarded buffer of a known bit pattern, two entries (rows) longer than N: every word outside reward[:N], done[:N], fired[:N],
    steps[:N] and columns < K of terms[:N] must keep its bits.  The gap columns of ``terms`` come back as ``fill``."""

    def run(storage, tb, rows, n, N, T, repr_, tsrcs, steps=None, max_steps=0, terms_ld=None, fill=0):
        dtype = storage.dtype
        table = Table(dm, tb)
        assert table.rc == 0, _lib.load().jxs_last_error()
        state = InNaN(storage)
        srcs = [None if s is None else InNaN(s[0]) for s in tsrcs]
        ld = tb.K if terms_ld is None else terms_ld
        pats = dict(reward=pattern_of(N + 2, dtype), done=pattern_of(N + 2, np.uint8), fired=pattern_of(N + 2, np.uint32),
                    terms=pattern_of((N + 2) * max(ld, 1), dtype), steps=pattern_of(N + 2, np.int32))  # fmt: skip
        if steps is not None:
            pats["steps"][:N] = steps
        bufs = {k: Guarded(v) for k, v in pats.items()}
        rc = env_evaluate(dm, table, state.ptr, [None if s is None else s.ptr for s in srcs], N, repr_, bufs["reward"].ptr, dtype, bufs["done"].ptr,
                          bufs["fired"].ptr, bufs["terms"].ptr if tb.K else None, dtype, ld, None if steps is None else bufs["steps"].ptr, max_steps)  # fmt: skip
        assert rc == 0, _lib.load().jxs_last_error()
        runtime.synchronize()
        out = {k: b.block() for k, b in bufs.items()}  # (checks the guards)
        for k in ("reward", "done", "fired", "steps"):
            same_words(out[k][N:], pats[k][N:], f"{k}: entries behind N - 1 were written")
        if steps is None:
            same_words(out["steps"], pats["steps"], "steps was written without being given")
        terms = out["terms"].reshape(N + 2, max(ld, 1))
        pt = pats["terms"].reshape(N + 2, max(ld, 1))
        assert_same_bits(terms[N:], pt[N:], "terms: rows behind N - 1 were written")
        assert_same_bits(np.ascontiguousarray(terms[:N, tb.K :]), np.ascontiguousarray(pt[:N, tb.K :]), "terms: the gap columns were written")
        res_terms = np.array(terms[:N, :ld]) if tb.K else np.zeros((N, 0), dtype)
        res_terms[:, tb.K :] = fill
        return dict(reward=np.array(out["reward"][:N]), done=np.array(out["done"][:N]), fired=np.array(out["fired"][:N]), terms=res_terms,
                    steps=None if steps is None else np.array(out["steps"][:N]))  # fmt: skip

    return run


def sizes_of(T):
    return sorted({1, T, 2 * T + 1})


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("key", MODELS)
def test_env_evaluate_keeps_the_contract_of_the_harness(models, key, dtype):
    """The checks of the host harness on the device (tests/test_env_evaluate_cpu.py::test_the_harness_equals_the_restatement:
    done, fired, steps and the bit-exact terms bit for bit against the NumPy restatement, ``EXP`` terms within 4 eps |want|,
    terms on derived kinds within their bounds of the float64 truth), over N in {1, T, 2T + 1} and the three representations,
    with every output in a guarded buffer.  Measured worst ratios over the four models: an ``EXP`` term 0.35 of 4 eps |want|
    (the device's exponential against NumPy's), a term on a derived kind 0.03 of its bound, the whole reward 0.01 of its."""
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    assert oref.n_rows(lay.n_joints, lay.n_points) == lay.n_rows
    worst = check_evaluate_against_the_restatement(device_evaluate(dm), lay.n_joints, lay.n_points, T, dtype, key, sizes=sizes_of(T))
    print("worst ratios:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("envs_per_wave", [8, 32])
def test_a_wave_of_several_tiles_and_a_partial_last_wave(models, knobs, envs_per_wave):
    """The developer knob asks for several tiles per wave at a small batch: the humanoid's N = 2T + 1 = 5 is then one wave of 8
    or 32 environments, partly empty."""
    knobs("JXS_EVALUATE_ENVS_PER_WAVE", envs_per_wave)
    model, dtype = sbc.build_model("icub", models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    check_evaluate_against_the_restatement(device_evaluate(dm), lay.n_joints, lay.n_points, T, dtype, f"E={envs_per_wave}", sizes=[2 * T + 1], seed=7)


def test_the_widest_table_in_fp64_on_the_largest_tile(models):
    """K + C = 64 in float64 on the model of the largest tile: (22 + 64) E words of 8 bytes per wave do not fit four times into
    64 KB, so the launcher runs two waves or one per workgroup."""
    dtype = np.float64
    key = max(MODELS, key=lambda k: runtime.device_model(sbc.build_model(k, models), dtype).layout.tile)
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    n, rows = lay.n_joints, lay.n_rows
    rng = np.random.default_rng(64)
    terms = [dict(slots=[(S, 0, int(r)) for r in rng.integers(0, rows, size=1 + t % 3)], inner=t % 4, weight=float(rng.uniform(-1, 1))) for t in range(32)]
    conds = [dict(slot=(S, 0, int(rng.integers(0, rows))), lo=-0.2 - 0.02 * c, kind=c % 2) for c in range(32)]
    tb = ref.make_table(terms, conds, termination_reward=-2.0)
    for N in (T + 1, 5 * T + 3):
        blk = make_block(n, lay.n_points, N, dtype, seed=N)
        steps = rng.integers(0, 9, size=N).astype(np.int32)
        want = ref.evaluate(blk, tb, n, oref.MIXED, steps=steps, max_steps=7)
        got = device_evaluate(dm)(oref.tile_block(blk, T, pad=np.nan), tb, rows, n, N, T, oref.MIXED, [None] * 3, steps=steps, max_steps=7)
        same_or_both_nan(got["reward"], want["reward"], np.ones(N, bool), f"{key} N={N} reward")
        same_or_both_nan(got["terms"], want["terms"], np.ones((N, 32), bool), f"{key} N={N} terms")
        for k in ("done", "fired", "steps"):
            assert np.array_equal(got[k], want[k]), f"{key} N={N}: {k}"
        assert want["fired"].max() >= 1 << 31 or N == T + 1


@pytest.mark.parametrize("key", ["icub", "quadruped_rigid"])
def test_the_kernel_equals_the_harness_and_reads_nothing_beyond_its_blocks(models, key):
    """State and sources lie between NaN words and their last tile is partly padding, also NaN: a word read beyond a block's
    storage, or from a padding column, would show in an output as NaN or as a fired condition.  Every output is finite and
    equals the harness's bit for bit in the bit-exact kinds."""
    model, dtype = sbc.build_model(key, models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    assert T > 1
    n, rows = lay.n_joints, lay.n_rows
    evaluate = device_evaluate(dm)
    eps = float(np.finfo(dtype).eps)
    for N in (1, T + 1, 2 * T + 1):  # (N % T = 1: T - 1 padding columns in the last tile)
        blk = make_block(n, lay.n_points, N, dtype, seed=N)
        blk[np.isnan(blk)] = 0.5  # (no NaN of the state's own)
        srcs = make_sources(N, dtype, seed=N)
        storage, tsrcs = oref.tile_block(blk, T, pad=np.nan), tiled_sources(srcs, T)
        steps = np.arange(N, dtype=np.int32)
        for repr_ in (oref.MIXED, oref.BODY):
            conds, margins = cond_list(n, blk, srcs, repr_)
            assert min(margins) > 1.0
            tb = ref.make_table(term_list(n, seed=rows), conds, reward_clip=(-3.0, 2.5), termination_reward=-1.25)
            got = evaluate(storage, tb, rows, n, N, T, repr_, tsrcs, steps=steps, max_steps=4, terms_ld=tb.K + 2, fill=0)
            want = emul.evaluate(storage, tb, rows, n, N, T, repr_, sources=tsrcs, steps=steps, max_steps=4)
            assert np.isfinite(got["reward"]).all() and np.isfinite(got["terms"]).all(), f"N={N}: a NaN from outside a block reached an output"
            exact, is_exp, is_derived = ref.term_classes(tb, repr_)
            gt = np.ascontiguousarray(got["terms"][:, : tb.K])
            same_or_both_nan(gt, want["terms"], np.broadcast_to(exact[None, :], gt.shape), f"{key} N={N} repr={repr_} terms")
            for k in ("done", "fired", "steps"):
                assert np.array_equal(got[k], want[k]), f"{key} N={N} repr={repr_}: {k}"
            # the other terms: kernel and harness each lie within the bound of the truth (4 eps |want| for an exponential)
            tol = 2 * ref.bounds(blk, tb, n, repr_, srcs) + 8 * eps * np.abs(want["terms"])
            assert (np.abs(gt.astype(np.float64) - want["terms"]) <= tol).all(), f"{key} N={N} repr={repr_}: kernel and harness disagree"


# ---- the Python layer -----------------------------------------------------------------------------------------------
def table_of(spec) -> ref.Table:
    return ref.Table(spec.slots, spec.offset, spec.scale, spec.targets, spec.terms, spec.term_params, spec.conditions, spec.condition_limits,
                     *spec.reward_clip, spec.termination_reward)  # fmt: skip


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_evaluate_equals_the_host_properties(models, dtype):
    N = 5
    model, blk, data = icub_data(models, N, dtype)
    eps = float(np.finfo(dtype).eps)
    z = float(np.sort(blk[2])[N // 2])  # (a height between the batch's: some environments lie below it)
    spec = js.data.RewardSpec.build(
        model,
        rewards=[("height", dict(term="base_height")), ("rate", dict(term="joint_velocities", inner="square", weight=-0.5)),
                 ("upright", dict(term="projected_gravity", index=2, weight=-1.0))],
        terminations=[("fell", dict(term="base_height", below=z))], termination_reward=-1.0, dtype=dtype)  # fmt: skip
    terms = DeviceMatrix(N, spec.n_terms, dtype)
    fired = DeviceWords(N)
    reward, done = data.evaluate(spec, terms=terms, fired=fired)
    assert isinstance(reward, DeviceMatrix) and reward.shape == (N, 1) and reward.dtype == dtype and isinstance(done, DeviceMask) and done.n == N
    t = terms.to_host()
    assert_same_bits(np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(data.base_position[:, 2]).astype(dtype), "height")
    qd = data.joint_velocities.astype(dtype)
    s = qd[:, 0] * qd[:, 0]
    for j in range(1, qd.shape[1]):
        s = s + qd[:, j] * qd[:, j]
    assert_same_bits(np.ascontiguousarray(t[:, 1]), (dtype(-0.5) * s).astype(dtype), "squared joint velocities, summed in joint order")
    R = data.base_transform[:, :3, :3].astype(np.float64)
    np.testing.assert_allclose(t[:, 2].astype(np.float64), R[:, 2, 2], rtol=0, atol=17 * eps)  # (-(R^T (0, 0, -1))_z = R_zz)
    below = data.base_position[:, 2].astype(dtype) < dtype(z)
    assert below.any() and not below.all()
    assert np.array_equal(done.to_host(), below.astype(np.uint8)) and np.array_equal(fired.to_host(), below.astype(np.uint32))
    want = ref.evaluate(blk, table_of(spec), model.dofs(), oref.MIXED)
    assert_same_bits(np.ascontiguousarray(t[:, :2]), np.ascontiguousarray(want["terms"][:, :2]), "the restatement")
    r = reward.to_host()[:, 0]
    total = ((t[:, 0] + t[:, 1]) + t[:, 2]) + np.where(below, dtype(-1.0), dtype(0.0))
    assert_same_bits(r, total.astype(dtype), "the reward is the sum of its terms in order, then the termination reward")
    # the returned mask goes into reset_where as it is
    fresh = js.data.JaxSimModelData.from_state_block(model, np.zeros_like(blk))
    after = data.reset_where(done, fresh).state_block()
    assert_same_bits(after, np.where(below[None, :], np.zeros_like(blk), blk), "reset_where(done)")


def test_foreign_outputs_are_written_in_place(models):
    N, dtype = 5, np.float64
    model, blk, data = icub_data(models, N, dtype)
    n = model.dofs()
    tau = DeviceArray.from_host(np.random.default_rng(2).uniform(-3, 3, (n, N)).astype(dtype), tile=data._state.tile)
    spec = js.data.RewardSpec.build(
        model, rewards=[("tau", dict(term=("source", dict(name="tau", rows=n)), inner="abs", weight=-0.1)), ("limits", dict(term="joint_positions", inner="excess"))],
        terminations=[("fell", dict(term="base_height", below=float(np.median(blk[2]))))], dtype=dtype)  # fmt: skip
    K, ld = spec.n_terms, spec.n_terms + 3
    own_r, own_d = data.evaluate(spec, sources={"tau": tau})
    own_t = DeviceMatrix(N, K, dtype)
    data.evaluate(spec, sources={"tau": tau}, terms=own_t)
    bufs = dict(terms=Guarded(pattern_of((N + 1) * ld, np.float32)), reward=Guarded(pattern_of(N, np.float32)), done=Guarded(pattern_of(N, np.uint8)),
                steps=Guarded(np.arange(N, dtype=np.int32) + 3))  # fmt: skip

    def foreign(shape, typestr, ptr, strides=None):
        class F:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}

        return F()

    f_terms = foreign((N, K), "<f4", bufs["terms"].ptr + 4, (ld * 4, 4))
    f_reward, f_done = foreign((N, 1), "<f4", bufs["reward"].ptr), foreign((N,), "|b1", bufs["done"].ptr)
    f_steps = foreign((N,), "<i4", bufs["steps"].ptr)
    r, d = data.evaluate(spec, sources={"tau": tau}, reward=f_reward, done=f_done, terms=f_terms, steps=f_steps, max_steps=6)
    assert r is f_reward and d is f_done
    runtime.synchronize()
    wide = bufs["terms"].block().reshape(N + 1, ld)
    assert_same_bits(np.ascontiguousarray(wide[:N, 1 : 1 + K]), own_t.to_host().astype(np.float32), "the foreign strided terms view, rounded once")
    rest = np.ones((N + 1, ld), bool)
    rest[:N, 1 : 1 + K] = False
    assert_same_bits(wide[rest], pattern_of((N + 1) * ld, np.float32).reshape(N + 1, ld)[rest], "words outside the view were written")
    assert_same_bits(bufs["reward"].block(), own_r.to_host()[:, 0].astype(np.float32), "the foreign reward")
    fell = own_d.to_host()
    st = np.arange(N, dtype=np.int32) + 4
    want_done = fell | np.where(st >= 6, 2, 0).astype(np.uint8)
    assert np.array_equal(bufs["done"].block(), want_done) and fell.any() and not fell.all()
    assert np.array_equal(bufs["steps"].block(), np.where(want_done != 0, 0, st))
    # this library's own vectors
    steps = DeviceIndices.from_host(np.arange(N) + 3)
    mask = DeviceMask(N)
    data.evaluate(spec, sources={"tau": tau}, done=mask, steps=steps, max_steps=6)
    assert np.array_equal(mask.to_host(), want_done) and np.array_equal(steps.to_host(), np.where(want_done != 0, 0, st))


# ---- the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_stream", [False, True], ids=["default-stream", "second-stream"])
def test_step_evaluate_reset_observe(models, second_stream):
    """20 iterations of step -> evaluate(steps, max_steps=7) -> reset_random_where(done) -> observe with nothing but device
    buffers, against the same loop whose reward, done and counters come from the NumPy restatement on state_block() downloads
    and whose mask is host bools: the final state, every step's reward and done and the counters agree bit for bit.  The terms
    are of the bit-exact kinds: a height window, the joint-limit excess, the squared joint velocities."""
    N, dtype, iters, max_steps = 6, np.float32, 20, 7
    model = sbc.build_model("icub", models)
    n = model.dofs()
    dist = js.data.RandomStateDistribution.build(model, dtype=dtype, **CONTACT)
    spec = js.data.RewardSpec.build(
        model,
        rewards=[("limits", dict(term="joint_positions", inner="excess", weight=-1.0)), ("rate", dict(term="joint_velocities", inner="square", weight=-1e-3)),
                 ("height", dict(term="base_height", offset=0.62, inner="abs", weight=-2.0))],
        terminations=[("height_window", dict(term="base_height", below=0.6, above=0.75))], termination_reward=-10.0, dtype=dtype)  # fmt: skip
    ospec = js.data.ObservationSpec.build(model, ["joint_positions", "joint_velocities", "base_height"], dtype=dtype)
    tb = table_of(spec)
    start = js.data.random_model_data_device(model, batch_size=N, dist=dist, draw=1000).state_block()
    make = js.data.JaxSimModelData.from_state_block
    # the host loop
    h = make(model, start)
    h_steps = np.zeros(N, np.int32)
    h_rewards, h_dones = [], []
    for k in range(iters):
        h = js.model.step(model, h, inplace=True)
        res = ref.evaluate(h.state_block(), tb, n, oref.MIXED, steps=h_steps, max_steps=max_steps)
        h_steps = res["steps"]
        h_rewards.append(res["reward"])
        h_dones.append(res["done"])
        h.reset_random_where(res["done"] != 0, dist, draw=k, inplace=True)
    h_obs = h.observe(ospec).to_host()
    want = h.state_block()
    all_done = np.concatenate(h_dones)
    assert (all_done & 1).any() and (all_done & 2).any(), "the case must see a termination and a truncation"
    assert np.isfinite(want).all() and np.isfinite(np.concatenate(h_rewards)).all()
    # the device loop
    stream = runtime.Stream() if second_stream else None
    runtime.synchronize()
    runtime.set_stream(stream)
    try:
        d = make(model, start)
        steps = DeviceIndices.from_host(np.zeros(N, np.int64))
        rewards = [DeviceMatrix(N, 1, dtype) for _ in range(iters)]
        dones = [DeviceMask(N) for _ in range(iters)]
        obs = DeviceMatrix(N, ospec.size, dtype)
        d.observe(ospec, out=obs)  # (uploads the tables before the loop)
        d.evaluate(spec, reward=rewards[0], done=dones[0])
        for k in range(iters):
            d = js.model.step(model, d, inplace=True)
            _, done = d.evaluate(spec, reward=rewards[k], done=dones[k], steps=steps, max_steps=max_steps)
            d.reset_random_where(done, dist, draw=k, inplace=True)
            d.observe(ospec, out=obs)
        runtime.synchronize()
        got = d.state_block()
        got_obs, got_steps = obs.to_host(), steps.to_host()
        got_rewards, got_dones = [r.to_host()[:, 0] for r in rewards], [m.to_host() for m in dones]
    finally:
        runtime.set_stream(None)
    for k in range(iters):
        assert np.array_equal(got_dones[k], h_dones[k]), f"done of iteration {k}"
        assert_same_bits(got_rewards[k], h_rewards[k], f"reward of iteration {k}")
    assert np.array_equal(got_steps, h_steps)
    assert_same_bits(got, want, "the loop through the device against the loop through the host")
    assert_same_bits(got_obs, h_obs, "the observation behind the loop")


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch(models):
    model, other = sbc.build_model("icub", models), sbc.build_model("cartpole", models)
    dtype, N = np.float32, 5
    _, blk, data = icub_data(models, N, dtype)
    lay = StateLayout.of(model)
    n = lay.n_joints
    tau = DeviceArray.from_host(np.random.default_rng(2).uniform(-3, 3, (n, N)).astype(dtype), tile=data._state.tile)
    build = js.data.RewardSpec.build
    spec = build(model, rewards=[("h", dict(term="base_height")), ("tau", dict(term=("source", dict(name="tau", rows=n)), inner="square"))],
                 terminations=[("fell", dict(term="base_height", below=float(np.median(blk[2]))))], dtype=dtype)  # fmt: skip
    K = spec.n_terms
    reward, done, terms, fired = DeviceMatrix(N, 1, dtype), DeviceMask(N), DeviceMatrix(N, K, dtype), DeviceWords(N)
    steps = DeviceIndices.from_host(np.arange(N))
    outs = dict(reward=reward, done=done, terms=terms, fired=fired, steps=steps, max_steps=9)
    data.evaluate(spec, sources={"tau": tau}, **outs)
    download = lambda: [reward.to_host(), done.to_host(), terms.to_host(), fired.to_host(), steps.to_host()]  # noqa: E731
    before = download()
    odata = js.data.JaxSimModelData.from_state_block(other, helpers.odata_to_block(other, models.random_data("cartpole", N, seed=1, dtype=dtype)))
    bad_calls = (
        lambda: odata.evaluate(spec, sources={"tau": tau}, **outs),
        lambda: data.evaluate(build(model, rewards=[("h", dict(term="base_height"))], dtype=np.float64), **outs),
        lambda: data.evaluate(spec, **outs),
        lambda: data.evaluate(spec, sources={"tau": DeviceArray(n + 1, N, dtype, tile=tau.tile)}, **outs),
        lambda: data.evaluate(spec, sources={"tau": tau, "more": tau}, **outs),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "reward": DeviceMatrix(N, 2, dtype)}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "done": DeviceMask(N + 1)}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "done": steps}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "terms": DeviceMatrix(N, K + 1, dtype)}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "fired": DeviceMask(N)}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "steps": DeviceWords(N)}),
        lambda: data.evaluate(spec, sources={"tau": tau}, **{**outs, "max_steps": 0}),
    )
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # the entry points themselves
    lib, dm, odm = _lib.load(), runtime.device_model(model, dtype), runtime.device_model(other, dtype)
    ok = [dict(slots=[(S, 0, 0), (S, 0, 1)])]
    for tb, word in (
        (ref.make_table([dict(slots=[(S, 0, lay.n_rows)])]), "row"), (ref.make_table([dict(slots=[(oref.SOURCE_ROW, 1, 0)])]), "source"),
        (ref.make_table([dict(slots=[(7, 0, 0)])]), "kind"), (ref.make_table([dict(slots=[(S, 0, 0)], target=(1, 0))]), "target"),
        (ref.make_table([dict(slots=[(S, 0, 0)], inner=4)]), "inner"), (ref.make_table([dict(slots=[(S, 0, 0)], outer=2)]), "outer"),
        (ref.make_table([dict(slots=[(S, 0, 0)], scale=np.inf)]), "finite"), (ref.make_table([dict(slots=[(S, 0, 0)], weight=1e39)]), "finite"),
        (ref.make_table([dict(slots=[(S, 0, 0)], lo=1.0, hi=0.0)]), "lo above hi"), (ref.make_table(ok, [dict(slot=(S, 0, 0), kind=2)]), "kind"),
        (ref.make_table(ok, [dict(slot=(S, 0, 0), lo=np.nan)]), "lo above hi"), (ref.make_table(ok, reward_clip=(1.0, 0.0)), "reward limits"),
        (ref.make_table(ok, termination_reward=np.inf), "termination_reward"), (ref.make_table([dict(slots=[(S, 0, 0)] * 1025)]), "outside"),
    ):  # fmt: skip
        t = Table(dm, tb)
        assert t.rc == -1 and t.handle.value is None and word in lib.jxs_last_error().decode() and b"jxs_evaluation_create" in lib.jxs_last_error(), lib.jxs_last_error()
    import dataclasses

    good = ref.make_table(ok + [dict(slots=[(S, 0, 2)])])
    for tb, word in ((dataclasses.replace(good, terms=np.array([(0, 2, 0, 0), (1, 2, 0, 0)], np.int32)), "overlaps"),
                     (dataclasses.replace(good, terms=np.array([(0, 2, 0, 0), (2, 0, 0, 0)], np.int32)), "empty"),
                     (dataclasses.replace(good, terms=np.array([(0, 1, 0, 0), (2, 1, 0, 0)], np.int32)), "belongs to no")):  # fmt: skip
        t = Table(dm, tb)
        assert t.rc == -1 and word in lib.jxs_last_error().decode(), lib.jxs_last_error()
    table = Table(dm, table_of(spec), source_rows=spec.source_rows)
    assert table.rc == 0, lib.jxs_last_error()
    st, src = data._state.ptr, [tau.ptr]
    full = dict(reward=reward.ptr, reward_dtype=dtype, done=done.ptr, fired=fired.ptr, terms=terms.ptr, terms_dtype=dtype, terms_ld=K, steps=steps.ptr, max_steps=9)
    call = lambda dm_=dm, st_=st, src_=src, N_=N, rep=2, **kw: env_evaluate(dm_, table, st_, src_, N_, rep, **{**full, **kw})  # noqa: E731
    assert call(terms_ld=K - 1) == -1 and b"terms_ld" in lib.jxs_last_error()
    assert call(rep=3) == -1 and b"representation" in lib.jxs_last_error()
    assert call(reward_dtype=np.float64) == -1 and b"reward_dtype" in lib.jxs_last_error()
    assert call(terms_dtype=np.float64) == -1 and b"terms_dtype" in lib.jxs_last_error()
    assert call(max_steps=0) == -1 and b"max_steps" in lib.jxs_last_error()
    assert call(reward=None, done=None) == -1 and b"at least one" in lib.jxs_last_error()
    assert call(src_=[None]) == -1 and b"source 0" in lib.jxs_last_error()
    assert call(N_=0) == -1
    assert call(dm_=odm) == -1 and b"another" in lib.jxs_last_error()
    assert call(st_=st + 2) == -1 and b"aligned" in lib.jxs_last_error()
    assert call(fired=fired.ptr + 2) == -1 and b"aligned" in lib.jxs_last_error()
    for got, was in zip(download(), before):
        same_words(got, was,"a refused call wrote an output")
    _lib.check(lib.jxs_memcpy_h2d(C.c_void_p(steps.ptr), np.arange(N, dtype=np.int32).ctypes.data_as(C.c_void_p), 4 * N, runtime._sp()), "h2d")
    assert call() == 0
    for got, was in zip(download(), before):
        same_words(got, was,"the same call, admitted")
