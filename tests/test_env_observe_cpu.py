"""The policy observation on the host: the harness (tests/env_observe_emul.py: jxs_obs::slot_value of
jaxsim_amd/csrc/jxs_env_observe.h over every word) against the NumPy restatement (tests/env_observe_ref.py) -- bit for bit in
the block's dtype for the kinds made of + - x, within bounds from the operation count against the float64 truth for the
rest --, the validity check of a slot table, the refusals of the entry points that need no device, and the host logic of
``js.data.ObservationSpec`` / ``JaxSimModelData.observe``."""

import ctypes as C

import numpy as np
import pytest

import env_observe_emul as emul
import env_observe_ref as ref
import jaxsim_amd.api as js
from env_cpu_support import check_observe_against_the_restatement, Foreign, lib, make_block, refused, REPRS, special_envs, stub_data  # noqa: F401  (lib: a fixture)
from jaxsim_amd import _lib, runtime
from jaxsim_amd.data import JaxSimModelData
from jaxsim_amd.model import VelRepr
from jaxsim_amd.state import StateLayout

DTYPES = (np.float32, np.float64)
SHAPES = ((23, 32), (12, 4), (2, 0), (0, 8))  # (n_joints, n_points)
TILES = (1, 2, 4)
GRID = [pytest.param(n, npt, T, dt, id=f"n{n}-p{npt}-T{T}-{np.dtype(dt).name}") for n, npt in SHAPES for T in TILES for dt in DTYPES]


def emul_observe(n, n_points, T):
    rows = ref.n_rows(n, n_points)

    def run(storage, slots, off, sc, N, repr_, tsrcs, out_ld, out_dtype):
        out = np.full(N * out_ld, np.nan, dtype=out_dtype)
        return emul.observe(storage, slots, off, sc, rows, n, N, T, repr_, sources=tsrcs, out=out, out_ld=out_ld, out_dtype=out_dtype).reshape(N, out_ld)

    return run


@pytest.mark.parametrize("n,n_points,T,dtype", GRID)
def test_the_harness_equals_the_restatement(n, n_points, T, dtype):
    """Bitwise for STATE_ROW, SOURCE_ROW, Inertial and Mixed velocity; within the bounds of the operation count for the unit
    quaternion (4 eps), the rotation entries and the projected gravity (16 eps absolute) and the Body velocity
    (64 eps (1 + |l| + |p||w|)).  Measured worst ratios of an error to its bound over this grid in float32: unit quaternion
    0.16, rotation 0.18, projected gravity 0.18, Body velocity 0.04; in float64 the harness and the truth are the same
    arithmetic and the ratios are 0."""
    worst = check_observe_against_the_restatement(emul_observe(n, n_points, T), n, n_points, T, dtype, "harness")
    print("worst error / bound per kind:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_zero_quaternion_and_a_nan_row_stay_where_they_are(dtype):
    n, n_points, T, N = 12, 4, 2, 5
    rows = ref.n_rows(n, n_points)
    slots = ref.full_table(rows, ())
    blk = make_block(n, n_points, N, dtype, seed=3)
    zero_q, nan_env = special_envs(n, N)
    nan_row = 7 + n // 2
    assert np.isnan(blk[nan_row, nan_env]) and (blk[3:7, zero_q] == 0).all()
    for repr_ in REPRS:
        got = emul.observe(ref.tile_block(blk, T, pad=np.nan), slots, 0.0, 1.0, rows, n, N, T, repr_)
        nan = np.isnan(got)
        assert nan[nan_env, nan_row] and nan.sum() == 1, "NaN outside the one slot of the one environment that holds it"
        z = got[zero_q]
        kind = slots[:, 0]
        np.testing.assert_array_equal(z[kind == ref.BASE_QUAT_UNIT], 0.0)  # (|q| = 0 leaves q as it is)
        np.testing.assert_array_equal(z[kind == ref.BASE_ROTATION].reshape(3, 3), np.eye(3))
        np.testing.assert_array_equal(z[kind == ref.PROJECTED_GRAVITY], [0.0, 0.0, -1.0])
        assert np.isfinite(z).all()


def test_the_validity_check_of_a_table():
    rows, src = 40, (5, 0, 3, 0)
    good = [(ref.STATE_ROW, 0, 0), (ref.STATE_ROW, 0, rows - 1), (ref.SOURCE_ROW, 0, 4), (ref.SOURCE_ROW, 2, 2), (ref.BASE_QUAT_UNIT, 0, 3),
            (ref.BASE_ROTATION, 0, 8), (ref.BASE_VELOCITY, 0, 5), (ref.PROJECTED_GRAVITY, 0, 2)]  # fmt: skip
    assert emul.table_error(good, rows, src) == ref.table_error(good, rows, src) == (ref.OK, -1)
    bad = {
        (ref.STATE_ROW, 0, rows): ref.BAD_INDEX, (ref.STATE_ROW, 0, -1): ref.BAD_INDEX,
        (ref.SOURCE_ROW, 0, 5): ref.BAD_INDEX, (ref.SOURCE_ROW, 2, 3): ref.BAD_INDEX, (ref.SOURCE_ROW, 2, -1): ref.BAD_INDEX,
        (ref.SOURCE_ROW, 1, 0): ref.BAD_SOURCE, (ref.SOURCE_ROW, 3, 0): ref.BAD_SOURCE, (ref.SOURCE_ROW, 4, 0): ref.BAD_SOURCE,
        (ref.SOURCE_ROW, -1, 0): ref.BAD_SOURCE,
        (ref.BASE_QUAT_UNIT, 0, 4): ref.BAD_INDEX, (ref.BASE_ROTATION, 0, 9): ref.BAD_INDEX, (ref.BASE_VELOCITY, 0, 6): ref.BAD_INDEX,
        (ref.PROJECTED_GRAVITY, 0, 3): ref.BAD_INDEX, (ref.BASE_ROTATION, 0, -1): ref.BAD_INDEX,
        (6, 0, 0): ref.BAD_KIND, (-1, 0, 0): ref.BAD_KIND,
    }  # fmt: skip
    for slot, code in bad.items():
        table = good + [slot]
        assert emul.table_error(table, rows, src) == ref.table_error(table, rows, src) == (code, len(good)), slot
    # a source of a table without source rows; the width
    assert emul.table_error([(ref.SOURCE_ROW, 0, 0)], rows, None)[0] == ref.BAD_SOURCE
    one = [(ref.STATE_ROW, 0, 1)]
    assert emul.table_error(one * ref.MAX_WIDTH, rows, src) == (ref.OK, -1)
    for D in (0, -1, ref.MAX_WIDTH + 1):
        assert emul.table_error(one, rows, src, D=D)[0] == ref.table_error(one, rows, src, D=D)[0] == ref.BAD_WIDTH
    assert emul.table_error([], rows, src)[0] == ref.BAD_WIDTH
    # an offset or a scale must be finite in the block's dtype
    for dtype in DTYPES:
        for v in (0.0, -3.5, float(np.finfo(dtype).max)):
            assert emul.affine_ok(v, dtype)
        for v in (np.inf, -np.inf, np.nan):
            assert not emul.affine_ok(v, dtype)
    assert not emul.affine_ok(1e39, np.float32) and emul.affine_ok(1e39, np.float64)
    # an invalid table or a null source is not evaluated
    blk = make_block(2, 0, 3, np.float32, seed=1)
    st = ref.tile_block(blk, 2)
    assert emul.observe(st, [(ref.STATE_ROW, 0, blk.shape[0])], 0, 1, blk.shape[0], 2, 3, 2, ref.MIXED, rc=True) == -2
    assert emul.observe(st, [(ref.SOURCE_ROW, 0, 0)], 0, 1, blk.shape[0], 2, 3, 2, ref.MIXED, sources=[None], rc=True) == -2
    # the derived values a launch computes: those the table reads, and the unit quaternion under every value made from it
    vel = [(ref.BASE_VELOCITY, 0, 0)]
    assert emul.derived_used(vel, ref.INERTIAL) == emul.derived_used(vel, ref.MIXED) == 1 << 13
    assert emul.derived_used(vel, ref.BODY) == (1 << 13) | 0xF
    assert emul.derived_used([(ref.PROJECTED_GRAVITY, 0, 2), (ref.STATE_ROW, 0, 3)], ref.MIXED) == (1 << 21) | 0xF
    assert emul.derived_used(one, ref.BODY) == 0


def test_cabi_exports_and_refusals_without_a_device(lib):  # noqa: F811
    for name in ("jxs_observation_create", "jxs_observation_destroy", "jxs_env_observe"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused before the model is looked at)
    slots = (C.c_int32 * 3)(0, 0, 0)
    h = C.c_void_p(0x2000)
    refused(lib, lib.jxs_observation_create(None, 1, slots, None, None, None, C.byref(h)), "null")
    assert h.value is None  # (a refused creation hands back no table)
    refused(lib, lib.jxs_observation_create(p, 1, slots, None, None, None, None), "null")
    refused(lib, lib.jxs_observation_create(p, 1, None, None, None, None, C.byref(h)), "null")
    assert lib.jxs_observation_destroy(None) == 0
    src = (C.c_void_p * 4)()
    for k in (0, 1, 2, 6):  # model, table, state, out
        args = [p, p, p, src, 3, 2, p, _lib.JXS_F32, 8, None]
        args[k] = None
        refused(lib, lib.jxs_env_observe(*args), "null")
    for N in (0, -1):
        refused(lib, lib.jxs_env_observe(p, p, p, src, N, 2, p, _lib.JXS_F32, 8, None), "positive")
    for rep in (-1, 3):
        refused(lib, lib.jxs_env_observe(p, p, p, src, 3, rep, p, _lib.JXS_F32, 8, None), "representation")


# ---- host logic of the Python layer ---------------------------------------------------------------------------------
def test_observation_spec_build(models):
    icub = models("icub")
    lay = StateLayout.of(icub)
    n = lay.n_joints
    names = icub.joint_names()
    pose = np.linspace(-0.5, 0.5, n)
    spec = js.data.ObservationSpec.build(
        icub,
        [("joint_positions", dict(offset=pose)), ("joint_velocities", dict(scale=0.05)), "base_orientation", "base_velocity", "projected_gravity",
         "base_height", ("source", dict(name="centroidal", rows=30, take=range(24), scale=2.0)), ("joint_positions", dict(joints=[names[3], names[0]], key="two")),
         "base_position", "base_quaternion", "base_rotation", "base_linear_velocity", "base_angular_velocity", "tangential_deformation"],
        velocity_representation=VelRepr.Body,
    )  # fmt: skip
    widths = [n, n, 4, 6, 3, 1, 24, 2, 3, 4, 9, 3, 3, 3 * lay.n_points]
    keys = ["joint_positions", "joint_velocities", "base_orientation", "base_velocity", "projected_gravity", "base_height", "centroidal", "two",
            "base_position", "base_quaternion", "base_rotation", "base_linear_velocity", "base_angular_velocity", "tangential_deformation"]  # fmt: skip
    assert spec.size == sum(widths) and list(spec.slices) == keys
    at = 0
    for key, w in zip(keys, widths):
        assert spec.slices[key] == slice(at, at + w), key
        at += w
    assert spec.dtype == np.float32 and spec.out_dtype == np.float32 and spec.velocity_representation == VelRepr.Body
    assert spec.layout == lay and spec.source_names == ("centroidal",) and spec.source_rows == (30,)
    s = spec.slots
    np.testing.assert_array_equal(s[spec.slices["joint_positions"]], [(ref.STATE_ROW, 0, lay.row_s + j) for j in range(n)])
    np.testing.assert_array_equal(s[spec.slices["joint_velocities"]], [(ref.STATE_ROW, 0, lay.row_sd + j) for j in range(n)])
    np.testing.assert_array_equal(s[spec.slices["two"]], [(ref.STATE_ROW, 0, lay.row_s + 3), (ref.STATE_ROW, 0, lay.row_s)])
    np.testing.assert_array_equal(s[spec.slices["base_orientation"]], [(ref.BASE_QUAT_UNIT, 0, c) for c in range(4)])
    np.testing.assert_array_equal(s[spec.slices["base_velocity"]], [(ref.BASE_VELOCITY, 0, c) for c in range(6)])
    np.testing.assert_array_equal(s[spec.slices["base_angular_velocity"]], [(ref.BASE_VELOCITY, 0, c) for c in range(3, 6)])
    np.testing.assert_array_equal(s[spec.slices["projected_gravity"]], [(ref.PROJECTED_GRAVITY, 0, c) for c in range(3)])
    np.testing.assert_array_equal(s[spec.slices["base_rotation"]], [(ref.BASE_ROTATION, 0, c) for c in range(9)])
    np.testing.assert_array_equal(s[spec.slices["base_height"]], [(ref.STATE_ROW, 0, 2)])
    np.testing.assert_array_equal(s[spec.slices["base_quaternion"]], [(ref.STATE_ROW, 0, 3 + c) for c in range(4)])
    np.testing.assert_array_equal(s[spec.slices["centroidal"]], [(ref.SOURCE_ROW, 0, r) for r in range(24)])
    np.testing.assert_array_equal(s[spec.slices["tangential_deformation"]], [(ref.STATE_ROW, 0, lay.row_m + r) for r in range(3 * lay.n_points)])
    np.testing.assert_array_equal(spec.offset[spec.slices["joint_positions"]], pose)
    assert (spec.scale[spec.slices["joint_velocities"]] == 0.05).all() and (spec.scale[spec.slices["centroidal"]] == 2.0).all()
    assert (spec.offset[n:] == 0).all() and (spec.scale[:n] == 1).all()
    assert ref.table_error(spec.slots, lay.n_rows, spec.source_rows) == emul.table_error(spec.slots, lay.n_rows, spec.source_rows) == (ref.OK, -1)
    # the defaults: the data object's representation at the call, out_dtype = dtype
    plain = js.data.ObservationSpec.build(icub, ["base_height"], dtype=np.float64)
    assert plain.size == 1 and plain.velocity_representation is None and plain.out_dtype == np.float64
    assert js.data.ObservationSpec.build(icub, ["base_height"], dtype=np.float64, out_dtype=np.float32).out_dtype == np.float32
    # four sources are the limit; a name may come back with the same rows
    four = [("source", dict(name=f"s{k}", rows=2 + k)) for k in range(4)]
    assert js.data.ObservationSpec.build(icub, four + [("source", dict(name="s1", rows=3, take=[2], key="again"))]).source_rows == (2, 3, 4, 5)
    build = js.data.ObservationSpec.build
    for bad in (
        [], ["nothing"], "base_height", [("joint_positions", dict(joints=["no_such_joint"]))], [("joint_positions", dict(offset=np.zeros(n + 1)))],
        [("base_height", dict(scale=np.inf))], [("base_height", dict(offset=np.nan))], [("base_height", dict(scale=1e39))], [("base_height", dict(gain=2))],
        ["base_height", "base_height"], [("source", dict(name="a"))], [("source", dict(name="a", rows=0))], [("source", dict(name="a", rows=3, take=[3]))],
        [("source", dict(name="a", rows=3)), ("source", dict(name="a", rows=4, key="b"))], four + [("source", dict(name="s4", rows=1))],
        [("joint_positions", dict(key=f"k{k}")) for k in range(4096 // n + 1)], [("base_height",)], [3],
    ):  # fmt: skip
        with pytest.raises(ValueError):
            build(icub, bad)
    for kw in (dict(dtype=np.float16), dict(dtype=np.float32, out_dtype=np.float64), dict(velocity_representation=7)):
        with pytest.raises(ValueError):
            build(icub, ["base_height"], **kw)
    # a model without joints has empty joint terms
    box = js.data.ObservationSpec.build(models("box"), ["joint_positions", "base_height"])
    assert box.size == 1 and box.slices["joint_positions"] == slice(0, 0)


def test_observe_refuses_mismatched_arguments_on_the_host(models):
    """The state of ``stub_data`` is no device buffer: every refusal comes before the first device call."""
    icub, cart = models("icub"), models("cartpole")
    N, T = 6, 2
    data = stub_data(icub, N, np.float32, tile=T)
    spec = js.data.ObservationSpec.build(icub, ["joint_positions", ("source", dict(name="cent", rows=5))])
    D = spec.size

    def block(rows=5, cols=N, dtype=np.float32, tile=T):
        b = runtime.DeviceArray.__new__(runtime.DeviceArray)  # (the metadata of a device array without a buffer)
        b.rows, b.cols, b.dtype, b.tile, b._ptr = rows, cols, np.dtype(dtype), tile, None
        return b

    good_out = Foreign((N, D), "<f4")
    for bad_spec in (js.data.ObservationSpec.build(cart, ["base_height"]), js.data.ObservationSpec.build(icub, ["base_height"], dtype=np.float64), "spec", None):
        with pytest.raises(ValueError):
            data.observe(bad_spec, out=good_out)
    for sources in (None, {}, {"other": block()}, {"cent": block(), "more": block()}, {"cent": block(rows=6)}, {"cent": block(cols=N + 1)},
                    {"cent": block(dtype=np.float64)}, {"cent": block(tile=4)}, {"cent": np.zeros((5, N), np.float32)}):  # fmt: skip
        with pytest.raises(ValueError):
            data.observe(spec, out=good_out, sources=sources)
    for out in (Foreign((N, D + 1), "<f4"), Foreign((N + 1, D), "<f4"), Foreign((N * D,), "<f4"), Foreign((N, D), "<f8"), Foreign((N, D), "<i4"),
                Foreign((N, D), "<f4", strides=(4 * D, 8)), Foreign((N, D), "<f4", strides=(4 * (D - 1), 4)), Foreign((N, D), "<f4", strides=(4 * D + 2, 4)),
                Foreign((N, D), "<f4", ptr=0), np.zeros((N, D), np.float32), "out"):  # fmt: skip
        with pytest.raises(ValueError):
            data.observe(spec, out=out, sources={"cent": block()})
    # what is accepted: a row stride, the data's own dtype
    assert runtime.foreign_matrix(Foreign((N, D), "<f4", ptr=0x3000, strides=(4 * (D + 3), 4)), N, D, ("<f4",)) == (0x3000, D + 3, np.dtype(np.float32))
    assert runtime.foreign_matrix(Foreign((N, D), "<f8", ptr=0x3000), N, D, ("<f4", "<f8")) == (0x3000, D, np.dtype(np.float64))
    assert isinstance(data, JaxSimModelData)
