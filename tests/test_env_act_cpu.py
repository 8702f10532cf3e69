"""The action-to-torque law without a device: the host harness (``jxs_act::torque_word`` of jaxsim_amd/csrc/jxs_env_act.h over
every word of the tiled torque block, tests/env_act_emul.py) against the NumPy restatement (tests/env_act_ref.py) bit for bit;
the validity check of a table; the refusals of the C ABI that need no device; ``js.data.ActionSpec.build`` and the host-side
refusals of ``JaxSimModelData.act``.

Only ``+ - x`` and comparisons are involved, so no tolerance exists.  The one freedom is the bit pattern of a NaN: an action
that is NaN, or an infinite one that meets ``inf - inf`` or ``0 x inf``, gives a NaN whose sign and payload are the
hardware's choice (x86 generates a negative quiet NaN, gfx950 a positive one), so two NaNs count as equal words."""

import ctypes as C

import numpy as np
import pytest

import env_act_emul as emul
import env_act_ref as ref
import jaxsim_amd.api as js
from env_cpu_support import check_act_against_the_restatement, Foreign, lib, make_action_table, make_case, refused, same_words, stub_data  # noqa: F401  (lib: a fixture)
from jaxsim_amd import _lib, runtime
from jaxsim_amd.state import StateLayout

DTYPES = (np.float32, np.float64)
SHAPES = ((23, 32), (12, 4), (2, 0), (1, 3))  # (n_joints, n_points)
TILES = (1, 2, 4)
GRID = [pytest.param(n, npt, T, dt, id=f"n{n}-p{npt}-T{T}-{np.dtype(dt).name}") for n, npt in SHAPES for T in TILES for dt in DTYPES]


def clamp_sides(blk, joints, params, actions, ff):
    """How often each clamp of the law cut from below, let through and cut from above (in float64, finite actions only)."""
    n = len(joints)
    q, qd = blk[ref.row_q(n) : ref.row_q(n) + n].astype(np.float64), blk[ref.row_qd(n) : ref.row_qd(n) + n].astype(np.float64)
    out = {"action": np.zeros(3, int), "target": np.zeros(3, int), "torque": np.zeros(3, int)}

    def count(key, x, lo, hi):
        x = x[np.isfinite(x)]
        out[key] += [(x < lo).sum(), ((x >= lo) & (x <= hi)).sum(), (x > hi).sum()]

    for j in range(n):
        (mode, column), p = joints[j], params[j]
        if column < 0:
            continue
        a = actions[:, column].astype(np.float64)
        if np.isfinite(p[ref.ACTION_CLIP]):
            count("action", a, -p[ref.ACTION_CLIP], p[ref.ACTION_CLIP])
        u = np.clip(a, -p[ref.ACTION_CLIP], p[ref.ACTION_CLIP]) * p[ref.SCALE] + p[ref.OFFSET]
        if mode == ref.POSITION and np.isfinite(p[ref.TARGET_LO]) and np.isfinite(p[ref.TARGET_HI]):
            count("target", u, p[ref.TARGET_LO], p[ref.TARGET_HI])
        if mode == ref.POSITION and np.isfinite(p[ref.TORQUE_LIMIT]):
            t = p[ref.KP] * (np.clip(u, p[ref.TARGET_LO], p[ref.TARGET_HI]) - q[j]) - p[ref.KD] * qd[j] + ff[j]
            count("torque", t, -p[ref.TORQUE_LIMIT], p[ref.TORQUE_LIMIT])
    return out


# ---- the harness against the restatement ----------------------------------------------------------------------------
def emul_act(n, n_points, T):
    def run(storage, joints, params, actions, A, N, ff):
        return emul.act(storage, joints, params, actions, ref.n_rows(n, n_points), N, T, A=A, feed_forward=ff)

    return run


@pytest.mark.parametrize("n,n_points,T,dtype", GRID)
def test_the_harness_equals_the_restatement(n, n_points, T, dtype):
    check_act_against_the_restatement(emul_act(n, n_points, T), n, n_points, T, dtype, "harness")


def test_every_clamp_is_met_from_both_sides_and_passed():
    """The cases of this module cut at every clamp from below and from above and also let values through."""
    blk, joints, params, actions, A, ff = make_case(23, 32, 37, np.float32, np.float32, seed=7 * 37)
    assert sorted(set(joints[:, 0])) == [ref.OFF, ref.TORQUE, ref.POSITION, ref.VELOCITY] and (joints[:, 1] == -1).any()
    assert len(set(range(A)) - set(joints[:, 1])) >= 1 and actions.shape[1] > A
    sides = clamp_sides(blk, joints, params, actions, ff)
    for key, counts in sides.items():
        assert (counts > 0).all(), (key, counts)
    # ... and on exactly this case the harness gives the restatement's words
    n, T, N = 23, 2, 37
    got = emul.act(ref.tile_block(blk, T, pad=np.nan), joints, params, actions, ref.n_rows(n, 32), N, T, A=A, feed_forward=ref.tile_block(ff, T, pad=np.nan))
    same_words(ref.untile_block(got, n, N, T)[0], ref.act(blk[7 : 7 + n], blk[13 + n : 13 + 2 * n], joints, params, actions, ff), "the case of the clamps")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_signed_zero_infinities_and_a_hold_entry(dtype):
    """One joint of each kind on values worked out by hand."""
    inf = np.inf
    joints = [(ref.TORQUE, 0), (ref.POSITION, -1), (ref.POSITION, 1), (ref.VELOCITY, 2), (ref.OFF, 3), (ref.TORQUE, 3)]
    #          scale offset  kp   kd  clip   lo    hi  limit
    params = [[1.0, -0.0, 0.0, 0.0, inf, -inf, inf, inf],  # -0 stays -0; +-inf pass an infinite limit
              [1.0, 0.25, 8.0, 0.5, inf, -inf, inf, inf],  # holds 0.25
              [2.0, 0.0, 4.0, 0.0, 0.5, -0.5, 0.75, 3.0],
              [1.0, 0.0, 0.0, 2.0, inf, -inf, inf, 1.5],
              [1.0, 0.0, 0.0, 0.0, inf, -inf, inf, inf],
              [1.0, -0.0, 0.0, 0.0, 0.0, -inf, inf, inf]]  # fmt: skip
    n, N, T = len(joints), 4, 2
    rows = ref.n_rows(n, 0)
    blk = np.zeros((rows, N), dtype)
    blk[ref.row_q(n) : ref.row_q(n) + n] = 0.5
    blk[ref.row_qd(n) : ref.row_qd(n) + n] = 1.0
    actions = np.array([[-0.0, 9.0, 0.25, 5.0], [inf, -9.0, 3.0, -5.0], [-inf, 0.125, 1.0, np.nan], [1.5, np.nan, -inf, -0.0]], np.float32)
    got, _ = ref.untile_block(emul.act(ref.tile_block(blk, T), joints, params, actions, rows, N, T), n, N, T)
    same_words(got, ref.act(blk[7 : 7 + n], blk[13 + n : 13 + 2 * n], joints, params, actions), "against the restatement")
    # joint 0: -0 x 1 + -0 = -0.  joint 1: 8 (0.25 - 0.5) - 0.5 x 1.  joint 2: 9 -> clip 0.5 -> u = 1 -> target 0.75 -> 4 x 0.25;
    # -9 -> u = -1 -> target -0.5 -> 4 x -1 = -4 -> limit -3; 0.125 -> u = 0.25 -> 4 x -0.25; NaN passes.  joint 3: 2 (u - 1):
    # -1.5 on the limit, 4 -> 1.5, 0, -inf -> -1.5.  joint 5, clamp(x, -0, 0) + -0: 5 -> 0 + -0 = 0; -5 -> -0; NaN; -0 stays -0
    want = np.array([
        [-0.0, inf, -inf, 1.5],
        [-2.5, -2.5, -2.5, -2.5],
        [1.0, -3.0, -1.0, np.nan],
        [-1.5, 1.5, 0.0, -1.5],
        [0.0, 0.0, 0.0, 0.0],
        [0.0, -0.0, np.nan, -0.0],
    ], dtype)  # fmt: skip
    same_words(got, want, "by hand")


def test_the_validity_check_of_a_table():
    good_j, good_p = make_action_table(9, 11, 3)
    for dt in DTYPES:
        assert ref.table_error(good_j, good_p, 11, dt) == emul.table_error(good_j, good_p, 11, dt) == (ref.OK, -1)
    cases = []  # (joint, change, code); every code at the first, a middle and the last joint

    def bad(j, code, column=None, mode=None, **p):
        cases.append((j, column, mode, p, code))

    for j in (0, 4, 8):
        for mode in (4, -1):
            bad(j, ref.BAD_MODE, mode=mode)
        for column in (11, -2):
            bad(j, ref.BAD_COLUMN, column=column)
        for k in (ref.SCALE, ref.OFFSET, ref.KP, ref.KD):
            for v in (np.nan, np.inf, -np.inf):
                bad(j, ref.NOT_FINITE, **{str(k): v})
        for k in (ref.ACTION_CLIP, ref.TORQUE_LIMIT):
            for v in (np.nan, -1.0, -np.inf, -1e-30):
                bad(j, ref.BAD_LIMIT, **{str(k): v})
        bad(j, ref.BAD_TARGETS, **{str(ref.TARGET_LO): 0.5, str(ref.TARGET_HI): 0.25})
        for k in (ref.TARGET_LO, ref.TARGET_HI):
            bad(j, ref.BAD_TARGETS, **{str(k): np.nan})
    for j, column, mode, p, code in cases:
        jj, pp = good_j.copy(), good_p.copy()
        if column is not None:
            jj[j, 1] = column
        if mode is not None:
            jj[j, 0] = mode
        for k, v in p.items():
            pp[j, int(k)] = v
        for dt in DTYPES:
            assert ref.table_error(jj, pp, 11, dt) == emul.table_error(jj, pp, 11, dt) == (code, j), (j, column, mode, p)
    # the first error wins; what is allowed: infinite limits, equal targets, infinite targets on the right side, A = 0 without columns
    jj, pp = good_j.copy(), good_p.copy()
    jj[2, 0], pp[1, ref.KP] = 9, np.nan
    assert emul.table_error(jj, pp, 11, np.float32) == ref.table_error(jj, pp, 11, np.float32) == (ref.NOT_FINITE, 1)
    pp = good_p.copy()
    pp[:, ref.TARGET_LO], pp[:, ref.TARGET_HI], pp[:, ref.ACTION_CLIP], pp[:, ref.TORQUE_LIMIT] = 0.5, 0.5, 0.0, np.inf
    pp[0, ref.TARGET_LO], pp[1, ref.TARGET_HI] = -np.inf, np.inf
    pp[2, ref.TARGET_LO] = pp[2, ref.TARGET_HI] = np.inf
    assert emul.table_error(good_j, pp, 11, np.float32) == ref.table_error(good_j, pp, 11, np.float32) == (ref.OK, -1)
    none = good_j.copy()
    none[:, 1] = -1
    for A, code in ((0, ref.OK), (4096, ref.OK), (-1, ref.BAD_WIDTH), (4097, ref.BAD_WIDTH)):
        assert emul.table_error(none, good_p, A, np.float32) == ref.table_error(none, good_p, A, np.float32) == (code, -1)
    assert emul.table_error(good_j, good_p, 11, np.float32, n=0) == ref.table_error(good_j, good_p, 11, np.float32, n=0) == (ref.BAD_JOINTS, -1)
    assert emul.table_error([], [], 3, np.float32) == (ref.BAD_JOINTS, -1)
    # finite in the block's type: 1e39 is a float64, no float32
    for k, code in ((ref.SCALE, ref.NOT_FINITE), (ref.KD, ref.NOT_FINITE), (ref.ACTION_CLIP, ref.BAD_LIMIT), (ref.TORQUE_LIMIT, ref.BAD_LIMIT),
                    (ref.TARGET_HI, ref.BAD_TARGETS)):  # fmt: skip
        pp = good_p.copy()
        pp[5, k] = 1e39
        assert emul.table_error(good_j, pp, 11, np.float64) == ref.table_error(good_j, pp, 11, np.float64) == (ref.OK, -1)
        assert emul.table_error(good_j, pp, 11, np.float32) == ref.table_error(good_j, pp, 11, np.float32) == (code, 5), k
    pp = good_p.copy()
    pp[5, ref.TARGET_LO] = -1e39
    assert emul.table_error(good_j, pp, 11, np.float32) == ref.table_error(good_j, pp, 11, np.float32) == (ref.BAD_TARGETS, 5)
    for dt in DTYPES:
        for v in (0.0, -0.0, 1.5, -3e38, 1e39, -1e39, 1e308, np.inf, -np.inf, np.nan):
            assert emul.finite_ok(v, dt) == ref.finite_in(v, dt), (v, dt)
            assert emul.limit_ok(v, dt) == ref.limit_ok(v, dt), (v, dt)
            for w in (0.0, 2.0, -np.inf, np.inf, np.nan, 1e39):
                assert emul.targets_ok(v, w, dt) == ref.targets_ok(v, w, dt), (v, w, dt)
    for mode in range(4):
        for column in (-1, 0, 1, 4095):
            assert emul.pack_roundtrip(mode, column)
    # the harness refuses what the entry point refuses
    blk, joints, params, actions, A, _ = make_case(9, 0, 3, np.float32, np.float32, 1)
    st = ref.tile_block(blk, 2)
    assert emul.act(st, joints, params, actions, ref.n_rows(9, 0), 3, 2, A=A, rc=True) == 0
    assert emul.act(st, joints, params, actions, ref.n_rows(9, 0), 3, 2, A=actions.shape[1] + 1, rc=True) == -2
    assert emul.act(st, joints, params, None, ref.n_rows(9, 0), 3, 2, A=A, rc=True) == -2


def test_cabi_exports_and_refusals_without_a_device(lib):  # noqa: F811
    for name in ("jxs_action_create", "jxs_action_destroy", "jxs_env_act"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused before the model is looked at)
    joints, params = (C.c_int32 * 2)(2, 0), (C.c_double * 8)(1, 0, 1, 1, 1, -1, 1, 1)
    h = C.c_void_p(0x2000)
    refused(lib, lib.jxs_action_create(None, 1, joints, params, C.byref(h)), "null")
    assert h.value is None  # (a refused creation hands back no table)
    refused(lib, lib.jxs_action_create(p, 1, joints, params, None), "null")
    refused(lib, lib.jxs_action_create(p, 1, None, params, C.byref(h)), "null")
    refused(lib, lib.jxs_action_create(p, 1, joints, None, C.byref(h)), "null")
    assert lib.jxs_action_destroy(None) == 0
    # jxs_env_act(model, table, state, actions, act_dtype, act_ld, feed_forward, out_tau, N, stream)
    for k in (0, 1, 2, 7):  # model, table, state, out
        args = [p, p, p, p, _lib.JXS_F32, 8, None, p, 3, None]
        args[k] = None
        refused(lib, lib.jxs_env_act(*args), "null")
    for N in (0, -1):
        refused(lib, lib.jxs_env_act(p, p, p, p, _lib.JXS_F32, 8, None, p, N, None), "positive")
    for dt in (-1, 2, 7):
        refused(lib, lib.jxs_env_act(p, p, p, p, dt, 8, None, p, 3, None), "act_dtype")


# ---- host logic of the Python layer ---------------------------------------------------------------------------------
def test_action_spec_build(models):
    icub = models("icub")
    lay = StateLayout.of(icub)
    n, names = lay.n_joints, list(icub.joint_names())
    build = js.data.ActionSpec.build
    # the defaults: every joint in model order, position mode, column j for joint j
    spec = build(icub, kp=40.0, kd=2.0)
    assert spec.layout == lay and spec.dtype == np.float32 and spec.width == n and spec.joint_names == tuple(names) and spec.reads_actions
    np.testing.assert_array_equal(spec.joints, [(ref.POSITION, j) for j in range(n)])
    np.testing.assert_array_equal(spec.params, np.tile([1.0, 0.0, 40.0, 2.0, np.inf, -np.inf, np.inf, np.inf], (n, 1)))
    assert ref.table_error(spec.joints, spec.params, spec.width, np.float32) == emul.table_error(spec.joints, spec.params, spec.width, np.float32) == (ref.OK, -1)
    # a subset in its own order, sequences, dicts, held joints, a wider tensor
    drive, held = [names[5], names[0], names[9]], {names[2]: 0.3, names[7]: -0.1}
    pose = np.array([0.1, -0.2, 0.3])
    spec = build(icub, dtype=np.float64, joints=drive, mode={names[0]: "velocity", names[9]: "torque"}, kp=[10.0, 20.0, 30.0], kd={names[5]: 0.5},
                 scale=0.25, offset=pose, action_clip=1.0, target_limits=(-0.5, {names[5]: 0.75}), torque_limit={names[5]: 60.0, names[2]: 7.0},
                 hold=held, hold_kp=100.0, hold_kd={names[7]: 3.0}, width=8)  # fmt: skip
    assert spec.dtype == np.float64 and spec.width == 8 and spec.joint_names == tuple(drive) and spec.columns == {names[5]: 0, names[0]: 1, names[9]: 2}
    want_j = np.full((n, 2), (ref.OFF, -1), np.int32)
    want_p = np.tile([1.0, 0.0, 0.0, 0.0, np.inf, -np.inf, np.inf, np.inf], (n, 1))
    want_j[5], want_j[0], want_j[9] = (ref.POSITION, 0), (ref.VELOCITY, 1), (ref.TORQUE, 2)
    want_p[5] = [0.25, 0.1, 10.0, 0.5, 1.0, -0.5, 0.75, 60.0]
    want_p[0] = [0.25, -0.2, 20.0, 0.0, 1.0, -0.5, np.inf, np.inf]
    want_p[9] = [0.25, 0.3, 30.0, 0.0, 1.0, -0.5, np.inf, np.inf]
    want_j[2], want_j[7] = (ref.POSITION, -1), (ref.POSITION, -1)
    want_p[2] = [1.0, 0.3, 100.0, 0.0, np.inf, -np.inf, np.inf, 7.0]
    want_p[7] = [1.0, -0.1, 100.0, 3.0, np.inf, -np.inf, np.inf, np.inf]
    np.testing.assert_array_equal(spec.joints, want_j)
    np.testing.assert_array_equal(spec.params, want_p)
    # the model's position limits as the target window; held joints take a scalar kp / kd and torque limit
    spec = build(icub, joints=drive, kp=5.0, kd=0.5, clip_to_position_limits=True, hold=held, torque_limit=9.0)
    lo, hi = js.joint.position_limits(icub)
    for j in (5, 0, 9):
        assert (spec.params[j, ref.TARGET_LO], spec.params[j, ref.TARGET_HI]) == (lo[j], hi[j])
    assert (spec.params[[2, 7], ref.KP] == 5.0).all() and (spec.params[[2, 7], ref.KD] == 0.5).all() and (spec.params[[0, 2, 5, 7, 9], ref.TORQUE_LIMIT] == 9.0).all()
    assert spec.params[1, ref.TORQUE_LIMIT] == np.inf and spec.joints[1, 0] == ref.OFF
    # per-joint gains without held joints: a sequence, a dict, both, over all joints and over a subset
    gains = np.linspace(10.0, 54.0, n)
    spec = build(icub, kp=list(gains))
    np.testing.assert_array_equal(spec.params[:, ref.KP], gains)
    assert (spec.params[:, ref.KD] == 0).all() and (spec.joints[:, 0] == ref.POSITION).all()
    spec = build(icub, kp=2.0, kd={names[4]: 3.0})
    want_kd = np.zeros(n)
    want_kd[4] = 3.0
    np.testing.assert_array_equal(spec.params[:, ref.KD], want_kd)
    assert (spec.params[:, ref.KP] == 2.0).all()
    spec = build(icub, joints=names[:3][::-1], kp=[1.0, 2.0, 3.0], kd={names[1]: 0.5}, hold_kp=None, hold_kd=None)
    np.testing.assert_array_equal(spec.params[:3, ref.KP], [3.0, 2.0, 1.0])
    np.testing.assert_array_equal(spec.params[:3, ref.KD], [0.0, 0.5, 0.0])
    np.testing.assert_array_equal(spec.joints[:4], [(ref.POSITION, 2), (ref.POSITION, 1), (ref.POSITION, 0), (ref.OFF, -1)])
    assert (spec.params[3:, ref.KP] == 0).all()
    # hold gains given without held joints are not looked at
    assert (build(icub, kp=list(gains), hold_kp=7.0, hold_kd={names[0]: 1.0}).params[:, ref.KP] == gains).all()
    # a spec without columns
    still = build(icub, joints=[], hold={nm: 0.0 for nm in names}, hold_kp=50.0, hold_kd=1.0)
    assert still.width == 0 and not still.reads_actions and (still.joints == (ref.POSITION, -1)).all()
    for kw in (
        dict(joints=["no_such_joint"]), dict(joints=names[0]), dict(joints=[names[0], names[0]]), dict(mode="servo"), dict(mode={names[0]: "servo"}),
        dict(mode={"no_such_joint": "torque"}), dict(joints=drive, hold={names[5]: 0.0}), dict(hold={"no_such_joint": 0.0}), dict(kp=np.inf), dict(kd=np.nan),
        dict(scale=1e39), dict(offset=[0.0] * (n - 1)), dict(kp={names[0]: np.nan}), dict(action_clip=-1.0), dict(action_clip=np.nan), dict(torque_limit=-0.5),
        dict(torque_limit=np.nan), dict(torque_limit=1e39), dict(target_limits=(0.5, 0.25)), dict(target_limits=(np.nan, 1.0)), dict(target_limits=(0.0,)),
        dict(target_limits=(-1.0, 1.0), clip_to_position_limits=True), dict(width=n - 1), dict(width=4097), dict(dtype=np.float16),
        dict(joints=drive, hold=held, kp=[1.0, 2.0, 3.0]), dict(joints=drive, hold={names[2]: np.nan}, hold_kp=1.0, hold_kd=1.0),
        dict(joints=drive, kd={names[1]: 1.0}),
    ):  # fmt: skip
        with pytest.raises(ValueError):
            build(icub, **kw)
    assert build(icub, scale=1e39, dtype=np.float64).params[0, ref.SCALE] == 1e39
    with pytest.raises(ValueError):
        build(models("box"))


def test_act_refuses_mismatched_arguments_on_the_host(models):
    """The state of ``stub_data`` is no device buffer: every refusal comes before the first device call."""
    icub, cart = models("icub"), models("cartpole")
    N, T = 6, 2
    data = stub_data(icub, N, np.float32, tile=T)
    n = StateLayout.of(icub).n_joints
    spec = js.data.ActionSpec.build(icub, kp=10.0, width=n + 2)
    A = spec.width

    def block(rows=n, cols=N, dtype=np.float32, tile=T):
        b = runtime.DeviceArray.__new__(runtime.DeviceArray)  # (the metadata of a device array without a buffer)
        b.rows, b.cols, b.dtype, b.tile, b._ptr = rows, cols, np.dtype(dtype), tile, None
        return b

    good = Foreign((N, A), "<f4")
    for bad_spec in (js.data.ActionSpec.build(cart, kp=1.0), js.data.ActionSpec.build(icub, dtype=np.float64), js.data.ObservationSpec.build(icub, ["base_height"]),
                     "spec", None):  # fmt: skip
        with pytest.raises(ValueError):
            data.act(bad_spec, good, out=block())
    for actions in (None, Foreign((N, A + 1), "<f4"), Foreign((N + 1, A), "<f4"), Foreign((N * A,), "<f4"), Foreign((N, A), "<f8"), Foreign((N, A), "<i4"),
                    Foreign((N, A), "<f4", strides=(4 * A, 8)), Foreign((N, A), "<f4", strides=(4 * (A - 1), 4)), Foreign((N, A), "<f4", ptr=0),
                    np.zeros((N, A + 1), np.float32), np.zeros((N - 1, A), np.float32), np.zeros(A, np.float32), np.zeros((N, A, 1))):  # fmt: skip
        with pytest.raises(ValueError):
            data.act(spec, actions, out=block())
    for kw in (dict(out=block(rows=n + 1)), dict(out=block(cols=N + 1)), dict(out=block(dtype=np.float64)), dict(out=block(tile=4)),
               dict(out=np.zeros((n, N), np.float32)), dict(out=block(), feed_forward=block(rows=n - 1)), dict(out=block(), feed_forward=block(tile=1)),
               dict(out=block(), feed_forward=np.zeros((n, N), np.float32))):  # fmt: skip
        with pytest.raises(ValueError):
            data.act(spec, good, **kw)
    # a read-only foreign tensor with a row stride is accepted for reading
    ro = Foreign((N, A), "<f4", ptr=0x3000, strides=(4 * (A + 3), 4))
    ro.__cuda_array_interface__["data"] = (0x3000, True)
    assert runtime.foreign_matrix(ro, N, A, ("<f4",), writable=False) == (0x3000, A + 3, np.dtype(np.float32))
    with pytest.raises(ValueError):
        runtime.foreign_matrix(ro, N, A, ("<f4",))
    with pytest.raises(ValueError):
        js.model.control_steps(icub, data, spec, good, 0)
