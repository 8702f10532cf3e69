"""The policy observation on the device: jxs_env_observe on guarded raw buffers against the checks the host harness is held
to (tests/test_env_observe_cpu.py: the NumPy restatement bit for bit for the + - x kinds, the float64 truth within the
bounds of the operation count for the rest) and against the harness itself; sources inside NaN surroundings; the Python
layer (``js.data.ObservationSpec`` / ``JaxSimModelData.observe``) against the host properties of the same data object; the
loop step -> observe -> policy -> step against the same loop through the host; refusals."""

import ctypes as C

import numpy as np
import pytest

import env_observe_emul as emul
import env_observe_ref as ref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from env_cpu_support import check_observe_against_the_restatement, make_block, make_sources, same_or_both_nan, SOURCE_ROWS, tiled_sources
from env_gpu_support import DTYPES, MODELS, Guarded, InNaN, assert_same_bits, icub_data, upload_flat
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceArray, DeviceMatrix
from jaxsim_amd.state import StateLayout

pytestmark = pytest.mark.gpu

class Table:
    """A ``jxs_observation`` of a device model, destroyed with the object."""

    def __init__(self, dm, slots, offset=None, scale=None, source_rows=SOURCE_ROWS):
        s = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1, 3)
        D = len(s)
        off = None if offset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(offset, np.float64), (D,)))
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (D,)))
        rows = (C.c_int32 * 4)(*(list(source_rows) + [0] * (4 - len(source_rows))))
        dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        self.handle, self.D = C.c_void_p(), D
        self.rc = _lib.load().jxs_observation_create(dm.handle, D, s.ctypes.data_as(C.POINTER(C.c_int32)), dp(off), dp(sc), rows, C.byref(self.handle))

    def __del__(self):
        if self.handle.value:
            _lib.load().jxs_observation_destroy(self.handle)


def env_observe(dm, table, state_ptr, source_ptrs, N, repr_, out_ptr, out_dtype, out_ld):
    ptrs = (C.c_void_p * 4)(*(list(source_ptrs) + [None] * (4 - len(source_ptrs))))
    return _lib.load().jxs_env_observe(dm.handle, table.handle, C.c_void_p(state_ptr), ptrs, N, repr_, C.c_void_p(out_ptr), _lib.dtype_code(out_dtype),
                                       out_ld, runtime._sp())  # fmt: skip


def device_observe(dm):
    """The ``observe`` of tests/test_env_observe_cpu.py::check_observe_against_the_restatement on the device.  The tensor lies in a
    guarded buffer of a known bit pattern, two rows longer than N: every word outside columns < D of rows < N must keep
    its bits -- the gap columns, the rows behind N - 1, the guards.  The gap columns come back as NaN."""

    def run(storage, slots, off, sc, N, repr_, tsrcs, out_ld, out_dtype):
        D = len(slots)
        table = Table(dm, slots, off, sc)
        assert table.rc == 0, _lib.load().jxs_last_error()
        state = InNaN(storage)
        srcs = [None if s is None else InNaN(s[0]) for s in tsrcs]
        u = np.uint32 if np.dtype(out_dtype) == np.float32 else np.uint64
        pattern = np.full((N + 2) * out_ld, 0x5A5A5A5A5A5A5A5A & np.iinfo(u).max, dtype=u).view(out_dtype)
        dst = Guarded(pattern)
        rc = env_observe(dm, table, state.ptr, [None if s is None else s.ptr for s in srcs], N, repr_, dst.ptr, out_dtype, out_ld)
        assert rc == 0, _lib.load().jxs_last_error()
        got = dst.block().reshape(N + 2, out_ld)  # (checks the guards)
        assert_same_bits(got[N:], pattern.reshape(N + 2, out_ld)[N:], "rows behind N - 1 were written")
        assert_same_bits(np.ascontiguousarray(got[:N, D:]), pattern.reshape(N + 2, out_ld)[:N, D:], "the gap columns were written")
        res = np.array(got[:N])
        res[:, D:] = np.nan
        return res

    return run


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("key", MODELS)
def test_env_observe_keeps_the_contract_of_the_harness(models, key, dtype):
    """The checks of the host harness on the device (state and source rows, Inertial and Mixed velocity bit for bit against
    the NumPy restatement, with and without offset / scale, into a wider row, fp32 from an fp64 block; unit quaternion,
    rotation, projected gravity and Body velocity within 4 eps / 16 eps / 16 eps / 64 eps (1 + |l| + |p||w|) of the float64
    truth), over N in {1, T, 2T + 1} and the three representations.  Measured worst ratios of an error to its bound in
    float32 over the four models: unit quaternion 0.14, rotation 0.20, projected gravity 0.16, Body velocity 0.03; in float64
    the kernel and the truth are the same arithmetic (0)."""
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    assert (dm.layout.n_rows, dm.layout.n_joints) == (lay.n_rows, lay.n_joints) and ref.n_rows(lay.n_joints, lay.n_points) == lay.n_rows
    worst = check_observe_against_the_restatement(device_observe(dm), lay.n_joints, lay.n_points, T, dtype, key)
    print("worst error / bound per kind:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("envs_per_wave", [8, 32])
def test_a_wave_of_several_tiles_and_a_partial_last_wave(models, knobs, envs_per_wave):
    """The launcher gives a wave more than one tile only for large batches; the developer knob asks for it at a small one:
    the humanoid's N = 2T + 1 = 5 is then one wave of 8 or 32 environments, partly empty."""
    knobs("JXS_OBSERVE_ENVS_PER_WAVE", envs_per_wave)
    model, dtype = sbc.build_model("icub", models), np.float32
    dm = runtime.device_model(model, dtype)
    lay = StateLayout.of(model)
    check_observe_against_the_restatement(device_observe(dm), lay.n_joints, lay.n_points, dm.layout.tile, dtype, f"E={envs_per_wave}", seed=7)


@pytest.mark.parametrize("key", ["icub", "quadruped_rigid"])
def test_the_kernel_equals_the_harness_and_reads_no_source_beyond_its_storage(models, key):
    """State and sources lie between NaN words and their last tile is partly padding, also NaN: a word read beyond a
    block's storage, or from a padding column, would show in the output as NaN.  The whole tensor equals the harness's
    bit for bit in the + - x kinds."""
    model, dtype = sbc.build_model(key, models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    assert T > 1
    n, rows = lay.n_joints, lay.n_rows
    slots = ref.full_table(rows, SOURCE_ROWS)
    observe = device_observe(dm)
    for N in (1, T + 1, 2 * T + 1):  # (N % T = 1: T - 1 padding columns in the last tile)
        blk = make_block(n, lay.n_points, N, dtype, seed=N)
        blk[np.isnan(blk)] = 0.5  # (no NaN of the state's own)
        srcs = make_sources(N, dtype, seed=N)
        storage, tsrcs = ref.tile_block(blk, T, pad=np.nan), tiled_sources(srcs, T)
        for repr_ in (ref.MIXED, ref.BODY):
            got = observe(storage, slots, 0.25, 2.0, N, repr_, tsrcs, len(slots) + 3, dtype)[:, : len(slots)]
            assert np.isfinite(got).all(), f"N={N}: a NaN from outside a block reached the output"
            want = emul.observe(storage, slots, 0.25, 2.0, rows, n, N, T, repr_, sources=tsrcs)
            exact = np.array([ref.bitwise(k, repr_) for k, _, _ in slots])
            same_or_both_nan(np.ascontiguousarray(got), want, np.broadcast_to(exact[None, :], got.shape), f"{key} N={N} repr={repr_}")
            # the other kinds: kernel and harness each lie within the bound of the truth, the slot scales by 2 and rounds twice
            tol = 2 * 2.0 * ref.bounds(slots, blk, n, dtype) + 4 * float(np.finfo(dtype).eps) * np.abs(want)
            assert (np.abs(got.astype(np.float64) - want) <= tol).all(), f"{key} N={N} repr={repr_}: kernel and harness disagree"


# ---- the Python layer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_observe_equals_the_host_properties(models, dtype):
    N = 5
    model, blk, data = icub_data(models, N, dtype)
    eps = float(np.finfo(dtype).eps)
    spec = js.data.ObservationSpec.build(model, ["joint_positions", "joint_velocities", "base_position", "base_quaternion"], dtype=dtype)
    obs = data.observe(spec)
    assert isinstance(obs, DeviceMatrix) and obs.shape == (N, spec.size) and obs.dtype == dtype
    assert obs.__cuda_array_interface__["shape"] == (N, spec.size) and obs.__cuda_array_interface__["typestr"] == np.dtype(dtype).str
    got = obs.to_host()
    assert got.shape == (N, spec.size)
    for name in ("joint_positions", "joint_velocities", "base_position", "base_quaternion"):
        assert_same_bits(np.ascontiguousarray(got[:, spec.slices[name]]), np.ascontiguousarray(getattr(data, name)), name)
    # the base velocity in the data object's representation at the call; unit quaternion, rotation
    vspec = js.data.ObservationSpec.build(model, ["base_velocity", "base_orientation", "base_rotation"], dtype=dtype)
    lay = StateLayout.of(model)
    b64 = blk.astype(np.float64)
    norm = lambda a: np.sqrt((a * a).sum(axis=0))  # noqa: E731
    vbound = 64 * eps * (1 + norm(b64[lay.row_vlin : lay.row_vlin + 3]) + norm(b64[0:3]) * norm(b64[lay.row_vang : lay.row_vang + 3]))
    for rep in (ja.VelRepr.Inertial, ja.VelRepr.Mixed, ja.VelRepr.Body):
        with data.switch_velocity_representation(rep):
            own = data.observe(vspec).to_host()
            want = np.asarray(data.base_velocity, np.float64)
        got = own.astype(np.float64)
        err = np.abs(got[:, vspec.slices["base_velocity"]] - want)
        assert (err <= vbound[:, None]).all(), (rep, float((err / vbound[:, None]).max()))
        # a spec that names its representation does not look at the data object's (Mixed here)
        pinned = js.data.ObservationSpec.build(model, ["base_velocity"], dtype=dtype, velocity_representation=rep)
        assert_same_bits(data.observe(pinned).to_host(), np.ascontiguousarray(own[:, vspec.slices["base_velocity"]]), f"pinned {rep}")
    np.testing.assert_allclose(got[:, vspec.slices["base_orientation"]], np.asarray(data.base_orientation, np.float64), rtol=0, atol=4 * eps)
    R = data.base_transform[:, :3, :3].reshape(N, 9).astype(np.float64)
    np.testing.assert_allclose(got[:, vspec.slices["base_rotation"]], R, rtol=0, atol=17 * eps)  # (16 eps, and the host's cast to dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_projected_gravity_of_a_known_roll_and_pitch(models, dtype):
    """R = Rz(yaw) Ry(pitch) Rx(roll): R^T (0, 0, -1) = (sin pitch, -cos pitch sin roll, -cos pitch cos roll), whatever the
    yaw.  Bound: the kernel's 16 eps, and 4 eps for the rounding of the stored quaternion (each component off by at most
    eps / 2 relative, the entries of R quadratic in them with coefficients of magnitude 2)."""
    model = sbc.build_model("icub", models)
    N = 5
    rng = np.random.default_rng(5)
    roll, pitch, yaw = rng.uniform(-1.2, 1.2, N), rng.uniform(-1.2, 1.2, N), rng.uniform(-3, 3, N)
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)
    data = js.data.JaxSimModelData.build(model, base_position=rng.uniform(-1, 1, (N, 3)), base_quaternion=q, dtype=dtype)
    spec = js.data.ObservationSpec.build(model, ["projected_gravity", "base_height"], dtype=dtype)
    got = data.observe(spec).to_host().astype(np.float64)
    want = np.stack([np.sin(pitch), -np.cos(pitch) * np.sin(roll), -np.cos(pitch) * np.cos(roll)], axis=1)
    np.testing.assert_allclose(got[:, spec.slices["projected_gravity"]], want, rtol=0, atol=20 * float(np.finfo(dtype).eps))
    assert_same_bits(np.ascontiguousarray(got[:, 3].astype(dtype)), np.ascontiguousarray(data.base_position[:, 2]), "base_height")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_source_and_a_foreign_output_with_a_row_stride(models, dtype):
    N = 5
    model, blk, data = icub_data(models, N, dtype)
    rec = js.com.centroidal_quantities(model, data)
    pose = np.linspace(-0.3, 0.3, model.dofs())
    spec = js.data.ObservationSpec.build(
        model, [("joint_positions", dict(offset=pose, scale=0.5)), ("source", dict(name="centroidal", rows=js.com.ROWS)), "base_height"], dtype=dtype)
    got = data.observe(spec, sources={"centroidal": rec}).to_host()
    rec_h = rec.to_host().T
    assert np.isfinite(rec_h).all() and np.abs(rec_h).max() > 0
    assert_same_bits(np.ascontiguousarray(got[:, spec.slices["centroidal"]]), np.ascontiguousarray(rec_h), "the centroidal record")
    s = data.joint_positions.astype(dtype)
    assert_same_bits(np.ascontiguousarray(got[:, spec.slices["joint_positions"]]), (s - pose.astype(dtype)) * dtype(0.5), "offset and scale")
    # out=: a foreign (N, D) view with a row stride inside a wider tensor, in float32 whatever the data's dtype
    D, ld = spec.size, spec.size + 5
    u = np.uint32
    pattern = np.full((N + 1) * ld, 0x5A5A5A5A, dtype=u).view(np.float32)
    dst = Guarded(pattern)

    class Foreign:
        __cuda_array_interface__ = {"shape": (N, D), "typestr": "<f4", "data": (dst.ptr + 2 * 4, False), "strides": (ld * 4, 4), "version": 3}

    out = Foreign()
    assert data.observe(spec, out=out, sources={"centroidal": rec}) is out
    wide = dst.block().reshape(N + 1, ld)
    assert_same_bits(np.ascontiguousarray(wide[:N, 2 : 2 + D]), got.astype(np.float32), "the foreign view")
    rest = np.ones((N + 1, ld), bool)
    rest[:N, 2 : 2 + D] = False
    assert_same_bits(wide[rest], pattern.reshape(N + 1, ld)[rest], "words outside the view were written")
    # a matrix of this library is written in place as well
    mine = DeviceMatrix(N, D, dtype)
    assert data.observe(spec, out=mine, sources={"centroidal": rec}) is mine
    assert_same_bits(mine.to_host(), got, "out=DeviceMatrix")


# ---- the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_stream", [False, True], ids=["default-stream", "second-stream"])
def test_step_observe_policy_step(models, second_stream):
    """20 iterations of step -> observe -> a PD torque computed on the device from the observation's buffer by a kernel that
    is not the product's (tests/policy_kernel.py, the stand-in for another framework's network) and handed back as a
    foreign tensor -> step, against the same loop with the torque computed on the host from data.joint_positions /
    data.joint_velocities: bit for bit.  On a second stream nothing synchronises inside the loop."""
    import policy_kernel

    N, dtype, steps = 6, np.float32, 20
    model, blk, _ = icub_data(models, N, dtype)
    n = model.dofs()
    q0 = blk[7 : 7 + n, 0].astype(dtype)  # (the pose of environment 0 as the set point)
    kp, kd = dtype(20.0), dtype(0.5)
    # the host loop
    h = js.data.JaxSimModelData.from_state_block(model, blk)
    for _ in range(steps):
        h = js.model.step(model, h, inplace=True)
        tau = (q0[None, :] - h.joint_positions.astype(dtype)) * kp - h.joint_velocities.astype(dtype) * kd
        h = js.model.step(model, h, joint_force_references=tau, inplace=True)
    want = h.state_block()
    # the device loop
    spec = js.data.ObservationSpec.build(model, ["joint_positions", "joint_velocities", "projected_gravity"], dtype=dtype)
    policy_kernel.lib()
    stream = runtime.Stream() if second_stream else None
    q0_d = upload_flat(q0)
    runtime.synchronize()
    runtime.set_stream(stream)
    try:
        d = js.data.JaxSimModelData.from_state_block(model, blk)
        obs = DeviceMatrix(N, spec.size, dtype)
        tau_d = DeviceMatrix(N, n, dtype)  # (the policy's output buffer; the step sees it as a foreign tensor)

        class Foreign:
            __cuda_array_interface__ = {"shape": (N, n), "typestr": "<f4", "data": (tau_d.ptr, False), "strides": None, "version": 3}

        d.observe(spec, out=obs)  # (uploads the table before the loop)
        for _ in range(steps):
            d = js.model.step(model, d, inplace=True)
            d.observe(spec, out=obs)
            policy_kernel.pd_torque(obs.ptr, spec.size, q0_d.ptr, n, N, float(kp), float(kd), tau_d.ptr, runtime._sp())
            d = js.model.step(model, d, joint_force_references=Foreign(), inplace=True)
        runtime.synchronize()
        got = d.state_block()
    finally:
        runtime.set_stream(None)
    assert np.isfinite(want).all()
    assert_same_bits(got, want, "the loop through the device against the loop through the host")


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch(models):
    model, other = sbc.build_model("icub", models), sbc.build_model("cartpole", models)
    dtype, N = np.float32, 5
    _, blk, data = icub_data(models, N, dtype)
    lay = StateLayout.of(model)
    spec = js.data.ObservationSpec.build(model, ["joint_positions", ("source", dict(name="cent", rows=js.com.ROWS))], dtype=dtype)
    rec = js.com.centroidal_quantities(model, data)
    D = spec.size
    obs = DeviceMatrix(N, D, dtype)
    data.observe(spec, out=obs, sources={"cent": rec})
    before = obs.to_host()
    odata = js.data.JaxSimModelData.from_state_block(other, helpers.odata_to_block(other, models.random_data("cartpole", N, seed=1, dtype=dtype)))
    bad_calls = (
        lambda: odata.observe(spec, out=obs, sources={"cent": rec}),
        lambda: data.observe(js.data.ObservationSpec.build(model, ["base_height"], dtype=np.float64), out=obs),
        lambda: data.observe(spec, out=obs),
        lambda: data.observe(spec, out=obs, sources={"cent": DeviceArray(js.com.ROWS + 1, N, dtype, tile=rec.tile)}),
        lambda: data.observe(spec, out=obs, sources={"cent": DeviceArray(js.com.ROWS, N + 1, dtype, tile=rec.tile)}),
        lambda: data.observe(spec, out=obs, sources={"cent": rec, "more": rec}),
        lambda: data.observe(spec, out=DeviceMatrix(N, D + 1, dtype), sources={"cent": rec}),
        lambda: data.observe(spec, out=DeviceMatrix(N + 1, D, dtype), sources={"cent": rec}),
        lambda: data.observe(spec, out=np.zeros((N, D), dtype), sources={"cent": rec}),
    )
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # the entry points themselves
    lib, dm, odm = _lib.load(), runtime.device_model(model, dtype), runtime.device_model(other, dtype)
    for slots, kw, word in (
        ([(ref.STATE_ROW, 0, lay.n_rows)], {}, "row"), ([(ref.BASE_ROTATION, 0, 9)], {}, "component"), ([(ref.SOURCE_ROW, 1, 0)], {}, "source"),
        ([(ref.SOURCE_ROW, 4, 0)], {}, "source"), ([(7, 0, 0)], {}, "kind"), ([(ref.STATE_ROW, 0, 0)] * (ref.MAX_WIDTH + 1), {}, "outside"),
        ([(ref.STATE_ROW, 0, 0)], dict(scale=np.inf), "finite"), ([(ref.STATE_ROW, 0, 0)], dict(offset=np.nan), "finite"),
        ([(ref.STATE_ROW, 0, 0)], dict(scale=1e39), "finite"),
    ):  # fmt: skip
        t = Table(dm, slots, **kw)
        assert t.rc == -1 and t.handle.value is None and word in lib.jxs_last_error().decode(), (slots[:1], lib.jxs_last_error())
    h = C.c_void_p()
    assert lib.jxs_observation_create(dm.handle, 0, (C.c_int32 * 3)(0, 0, 0), None, None, None, C.byref(h)) == -1 and b"outside" in lib.jxs_last_error()
    table = Table(dm, spec.slots, spec.offset, spec.scale, source_rows=spec.source_rows)
    assert table.rc == 0
    st, src = data._state.ptr, [rec.ptr]
    assert env_observe(dm, table, st, src, N, 2, obs.ptr, dtype, D - 1) == -1 and b"out_ld" in lib.jxs_last_error()
    assert env_observe(dm, table, st, src, N, 3, obs.ptr, dtype, D) == -1 and b"representation" in lib.jxs_last_error()
    assert env_observe(dm, table, st, src, N, 2, obs.ptr, np.float64, D) == -1 and b"out_dtype" in lib.jxs_last_error()
    assert lib.jxs_env_observe(dm.handle, table.handle, C.c_void_p(st), (C.c_void_p * 4)(rec.ptr), N, 2, C.c_void_p(obs.ptr), 7, D, None) == -1
    assert env_observe(dm, table, st, [None], N, 2, obs.ptr, dtype, D) == -1 and b"source 0" in lib.jxs_last_error()
    assert lib.jxs_env_observe(dm.handle, table.handle, C.c_void_p(st), None, N, 2, C.c_void_p(obs.ptr), 0, D, None) == -1
    assert env_observe(dm, table, st, src, 0, 2, obs.ptr, dtype, D) == -1
    assert env_observe(odm, table, st, src, N, 2, obs.ptr, dtype, D) == -1 and b"another" in lib.jxs_last_error()
    assert env_observe(dm, table, st + 2, src, N, 2, obs.ptr, dtype, D) == -1 and b"aligned" in lib.jxs_last_error()
    assert_same_bits(obs.to_host(), before, "a refused call wrote the tensor")
    assert env_observe(dm, table, st, src, N, 2, obs.ptr, dtype, D) == 0
    assert_same_bits(obs.to_host(), before, "the same call, admitted")
