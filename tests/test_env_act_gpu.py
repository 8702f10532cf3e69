"""The action-to-torque law on the device: jxs_env_act on guarded raw buffers against the host harness and the NumPy
restatement, bit for bit (same_words of tests/env_cpu_support.py: two NaNs are the same word); state and feed-forward inside NaN
surroundings with NaN padding columns, the action tensor at the end of its upload with NaN in the gap and in unnamed columns;
waves of several tiles and a tensor of the widest kind; the Python layer (``js.data.ActionSpec`` /
``JaxSimModelData.act`` / ``js.model.control_steps``) against the restatement fed from the host properties; the decimation
loop against the same loop through the host; refusals."""

import ctypes as C

import numpy as np
import pytest

import env_act_emul as emul
import env_act_ref as ref
import helpers
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from env_cpu_support import bits, check_act_against_the_restatement, make_case, same_words
from env_gpu_support import DTYPES, Guarded, InNaN, assert_same_bits, icub_data, upload_flat
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceArray, DeviceMatrix
from jaxsim_amd.state import StateLayout

pytestmark = pytest.mark.gpu

JOINTED = ("icub", "quadruped_rigid", "cartpole")  # humanoid (T = 2, n = 23), quadruped, cartpole (fixed base, large T)


class Table:
    """A ``jxs_action`` of a device model, destroyed with the object."""

    def __init__(self, dm, joints, params, A):
        j = np.ascontiguousarray(joints, dtype=np.int32).reshape(-1, 2)
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 8)
        self.handle = C.c_void_p()
        self.rc = _lib.load().jxs_action_create(dm.handle, A, j.ctypes.data_as(C.POINTER(C.c_int32)), p.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.byref(self.handle))  # fmt: skip

    def __del__(self):
        if self.handle.value:
            _lib.load().jxs_action_destroy(self.handle)


def env_act(dm, table, state_ptr, act_ptr, act_dtype, act_ld, ff_ptr, out_ptr, N):
    vp = lambda p: None if p is None else C.c_void_p(p)  # noqa: E731
    return _lib.load().jxs_env_act(dm.handle, table.handle, vp(state_ptr), vp(act_ptr), _lib.dtype_code(act_dtype), act_ld, vp(ff_ptr), vp(out_ptr), N,
                                   runtime._sp())  # fmt: skip


def device_act(dm, n):
    """The ``act`` of tests/env_cpu_support.py::check_act_against_the_restatement on the device.  The torque block lies in a
    guarded buffer of a known bit pattern; the action tensor ends where its upload ends (a row read at or beyond N would lie
    outside it); state and feed-forward lie between NaN words.  The result is also held against the harness."""
    T = dm.layout.tile

    def run(storage, joints, params, actions, A, N, ff):
        table = Table(dm, joints, params, A)
        assert table.rc == 0, _lib.load().jxs_last_error()
        state = InNaN(storage)
        ffb = None if ff is None else InNaN(ff)
        acts = upload_flat(np.ascontiguousarray(actions).reshape(-1))
        words = -(-N // T) * n * T
        u = np.uint32 if storage.dtype == np.float32 else np.uint64
        dst = Guarded(np.full(words, 0x5A5A5A5A5A5A5A5A & np.iinfo(u).max, dtype=u).view(storage.dtype))
        rc = env_act(dm, table, state.ptr, acts.ptr, actions.dtype, actions.shape[1], None if ffb is None else ffb.ptr, dst.ptr, N)
        assert rc == 0, _lib.load().jxs_last_error()
        got = np.array(dst.block())  # (checks the guards)
        same_words(got, emul.act(storage, joints, params, actions, dm.layout.n_rows, N, T, A=A, feed_forward=ff), f"N={N}: kernel against harness")
        return got

    return run


def sizes_of(T, key):
    return sorted({1, T - 1, T + 1, 9 * T + 1} - {0}) + ([1001] if key == "icub" else [])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("key", JOINTED)
def test_env_act_equals_the_harness_and_the_restatement(models, key, dtype):
    """Every word of the torque block over N in {1, T - 1, T + 1, 9 T + 1} (and about 1000 on the humanoid): a ragged last
    tile, fewer environments than a tile, more than one workgroup; float32 and same-dtype actions; with and without
    feed-forward.  The guards are intact, the padding columns +0, every other word that of the harness and of the restatement."""
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    assert (dm.layout.n_rows, dm.layout.n_joints) == (lay.n_rows, lay.n_joints) and ref.n_rows(lay.n_joints, lay.n_points) == lay.n_rows
    check_act_against_the_restatement(device_act(dm, lay.n_joints), lay.n_joints, lay.n_points, T, dtype, key, sizes=sizes_of(T, key))


@pytest.mark.parametrize("envs_per_wave", [8, 32])
def test_waves_of_several_tiles_and_a_partial_last_wave(models, knobs, envs_per_wave):
    """The launcher gives a wave more than one tile only for large batches; the developer knob asks for it at small ones:
    the humanoid's N = 9 T + 1 = 19 is then three waves of 8 or one of 32 environments, the last partly empty."""
    knobs("JXS_ACT_ENVS_PER_WAVE", envs_per_wave)
    for key, dtype in (("icub", np.float32), ("icub", np.float64), ("cartpole", np.float32)):
        model = sbc.build_model(key, models)
        dm = runtime.device_model(model, dtype)
        lay = StateLayout.of(model)
        check_act_against_the_restatement(device_act(dm, lay.n_joints), lay.n_joints, lay.n_points, dm.layout.tile, dtype, f"{key} E={envs_per_wave}",
                                      seed=11, sizes=(1, dm.layout.tile + 1, 9 * dm.layout.tile + 1))  # fmt: skip


def test_a_misaligned_block_takes_narrower_accesses_and_a_spec_without_columns_needs_no_tensor(models):
    """A torque block at an address that is a multiple of 4 but not of 8 makes the humanoid's fp32 launch fall back from 8-
    to 4-byte accesses; a table without columns takes NULL actions."""
    model, dtype = sbc.build_model("icub", models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    n, N = lay.n_joints, 2 * T + 1
    blk, joints, params, actions, A, ff = make_case(n, lay.n_points, N, dtype, dtype, seed=5)
    storage = ref.tile_block(blk, T, pad=np.nan)
    want = emul.act(storage, joints, params, actions, lay.n_rows, N, T, A=A)
    table, state, acts = Table(dm, joints, params, A), InNaN(storage), upload_flat(np.ascontiguousarray(actions).reshape(-1))
    words = -(-N // T) * n * T
    dst = Guarded(np.full(words + 1, 7.0, dtype))
    assert env_act(dm, table, state.ptr, acts.ptr, dtype, actions.shape[1], None, dst.ptr + 4, N) == 0, _lib.load().jxs_last_error()
    got = np.array(dst.block())
    assert got[0] == 7.0
    same_words(got[1:], want, "an odd word address")
    # no joint has a column: hold entries and off
    joints2 = joints.copy()
    joints2[:, 1] = -1
    table2 = Table(dm, joints2, params, 0)
    assert table2.rc == 0
    dst = Guarded(np.full(words, 7.0, dtype))
    assert env_act(dm, table2, state.ptr, None, dtype, 0, None, dst.ptr, N) == 0, _lib.load().jxs_last_error()
    same_words(np.array(dst.block()), emul.act(storage, joints2, params, None, lay.n_rows, N, T, A=0), "no columns")


@pytest.mark.parametrize("width,envs_per_wave", [(4096, 0), (4096, 32)])
def test_the_widest_action_tensor(models, knobs, width, envs_per_wave):
    """4096 columns, the named ones spread over the whole row, the last one at its end."""
    knobs("JXS_ACT_ENVS_PER_WAVE", envs_per_wave or None)
    model, dtype = sbc.build_model("icub", models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    n, N = lay.n_joints, 9 * T + 1
    blk, joints, params, small, A, ff = make_case(n, lay.n_points, N, dtype, dtype, seed=13)
    spread = (width - 1) // (A - 1)  # column c of the small tensor becomes column c * spread, the last one width - 1 or near it
    actions = np.full((N, width), np.nan, dtype)
    actions[:, : A * spread : spread] = small[:, :A]
    joints = joints.copy()
    joints[:, 1] = np.where(joints[:, 1] >= 0, joints[:, 1] * spread, -1)
    storage, ff_t = ref.tile_block(blk, T, pad=np.nan), ref.tile_block(ff, T, pad=np.nan)
    got = device_act(dm, n)(storage, joints, params, actions, width, N, ff_t)
    tau, pad = ref.untile_block(got, n, N, T)
    same_words(tau, ref.act(blk[7 : 7 + n], blk[13 + n : 13 + 2 * n], joints, params, actions, ff), f"A = {width}")
    assert (bits(pad) == 0).all()


# ---- the Python layer -----------------------------------------------------------------------------------------------
def icub_spec(model, dtype, width=None):
    names = list(model.joint_names())
    drive = names[3:] + names[:1]  # (a column order that is not the model's)
    hold = {names[1]: 0.2}
    return js.data.ActionSpec.build(model, dtype=dtype, joints=drive, mode={names[4]: "velocity", names[5]: "torque"}, kp=30.0, kd=1.5, scale=0.5,
                                    offset=np.linspace(-0.3, 0.3, len(drive)), action_clip=1.0, clip_to_position_limits=True, torque_limit=25.0, hold=hold,
                                    hold_kp=80.0, hold_kd=2.0, width=width)  # fmt: skip


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_act_equals_the_restatement_fed_from_the_host_properties(models, dtype):
    N = 5
    model, blk, data = icub_data(models, N, dtype)
    n = model.dofs()
    spec = icub_spec(model, dtype, width=n + 3)
    A = spec.width
    rng = np.random.default_rng(3)
    actions = np.full((N, A), np.nan, np.float32)
    actions[:, : len(spec.joint_names)] = rng.normal(0, 1.2, (N, len(spec.joint_names)))
    q, qd = np.ascontiguousarray(data.joint_positions.T.astype(dtype)), np.ascontiguousarray(data.joint_velocities.T.astype(dtype))
    want = ref.act(q, qd, spec.joints, spec.params, actions)
    assert np.isfinite(want).all() and (want[2] == 0).all() and (np.abs(want) == 25.0).any() and (np.abs(want) < 25.0).any()
    # a DeviceMatrix, a host array, a strided read-only foreign float32 matrix inside a wider tensor
    tau = data.act(spec, DeviceMatrix.from_host(actions))
    assert isinstance(tau, DeviceArray) and tau.shape == (n, N) and tau.dtype == dtype and tau.tile == data._state.tile
    assert_same_bits(tau.to_host(), want, "DeviceMatrix")
    assert_same_bits(data.act(spec, actions).to_host(), want, "host array")
    ld = A + 4
    wide = np.full((N + 1, ld), np.nan, np.float32)
    wide[:N, 2 : 2 + A] = actions
    buf = upload_flat(wide.reshape(-1)[: N * ld - (ld - 2 - A)])  # (the upload ends with the last word of the view)

    class Foreign:
        __cuda_array_interface__ = {"shape": (N, A), "typestr": "<f4", "data": (buf.ptr + 2 * 4, True), "strides": (ld * 4, 4), "version": 3}

    out = DeviceArray(n, N, dtype, tile=data._state.tile)
    assert data.act(spec, Foreign(), out=out) is out
    assert_same_bits(out.to_host(), want, "foreign view")
    # actions of the data's own dtype; a feed-forward block
    ff_h = rng.uniform(-3, 3, (n, N)).astype(dtype)
    ff = DeviceArray.from_host(ff_h, tile=data._state.tile)
    assert_same_bits(data.act(spec, actions.astype(dtype), feed_forward=ff).to_host(), ref.act(q, qd, spec.joints, spec.params, actions.astype(dtype), ff_h), "feed-forward")
    # the result goes straight into step
    stepped = js.model.step(model, data, joint_force_references=tau).state_block()
    assert_same_bits(stepped, js.model.step(model, data, joint_force_references=want.T.copy()).state_block(), "step(joint_force_references=act(...))")
    # a spec without columns takes None
    still = js.data.ActionSpec.build(model, dtype=dtype, joints=[], hold={nm: 0.1 for nm in model.joint_names()}, hold_kp=40.0, hold_kd=1.0)
    assert_same_bits(data.act(still, None).to_host(), ref.act(q, qd, still.joints, still.params, None), "hold everything")


def test_one_spec_serves_two_device_models_of_one_layout_with_one_table(models, monkeypatch):
    """One ``ActionSpec`` used on two ``JaxSimModel`` objects built separately from the same description, hence on two device
    models of one layout: the torque block is, bit for bit, that of a spec per model, and the shared spec uploads exactly one
    table.  The cartpole, the smallest jointed model here, with N = 3: a last tile with padding columns."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    dtype, N = np.float32, 3
    first, second = (ja.JaxSimModel.build_from_model_description(robots.cartpole_urdf()) for _ in range(2))
    dms = [runtime.device_model(m, dtype) for m in (first, second)]
    assert first is not second and dms[0] is not dms[1]
    assert N % dms[0].layout.tile != 0
    blk = helpers.odata_to_block(first, models.random_data("cartpole", N, seed=7, dtype=dtype))
    actions = DeviceMatrix.from_host(np.random.default_rng(5).normal(0, 1.2, (N, first.dofs())).astype(np.float32))

    def spec_of(model):
        return js.data.ActionSpec.build(model, dtype=dtype, kp=30.0, kd=1.5, scale=0.5, action_clip=1.0, torque_limit=4.0)

    lib, created = _lib.load(), []
    create = lib.jxs_action_create
    monkeypatch.setattr(lib, "jxs_action_create", lambda *args: created.append(args) or create(*args))
    shared = spec_of(first)
    data = [js.data.JaxSimModelData.from_state_block(m, blk) for m in (first, second)]
    got = [d.act(shared, actions).to_host_raw() for d in data]
    assert len(created) == 1, "the shared spec uploaded more than one table"
    for k, (m, d) in enumerate(zip((first, second), data)):
        want = d.act(spec_of(m), actions).to_host_raw()
        assert np.isfinite(want).all() and (want != 0).any()
        assert_same_bits(got[k], want, f"the shared spec on model {k} against a spec of its own")
    assert len(created) == 3


@pytest.mark.parametrize("second_stream", [False, True], ids=["default-stream", "second-stream"])
def test_control_steps_equals_the_loop_through_the_host(models, second_stream):
    """Five policy steps of ``control_steps`` with decimation 2 (on a second stream nothing synchronises inside), against the
    same loop with the torques computed on the host by the restatement from the data object's properties and handed to
    ``step`` as host arrays: bit for bit."""
    N, dtype, policy_steps, decimation = 6, np.float32, 5, 2
    model, blk, _ = icub_data(models, N, dtype)
    n = model.dofs()
    spec = icub_spec(model, dtype)
    rng = np.random.default_rng(9)
    acts = rng.normal(0, 1.0, (policy_steps, N, spec.width)).astype(np.float32)
    ff_h = rng.uniform(-1, 1, (n, N)).astype(dtype)
    # the host loop
    h = js.data.JaxSimModelData.from_state_block(model, blk)
    for k in range(policy_steps):
        for _ in range(decimation):
            q, qd = np.ascontiguousarray(h.joint_positions.T.astype(dtype)), np.ascontiguousarray(h.joint_velocities.T.astype(dtype))
            tau = ref.act(q, qd, spec.joints, spec.params, acts[k], ff_h)
            h = js.model.step(model, h, joint_force_references=tau.T.copy(), inplace=True)
    want = h.state_block()
    # the device loop
    stream = runtime.Stream() if second_stream else None
    runtime.synchronize()
    runtime.set_stream(stream)
    try:
        d = js.data.JaxSimModelData.from_state_block(model, blk)
        ff = DeviceArray.from_host(ff_h, tile=d._state.tile)
        mats = [DeviceMatrix.from_host(a) for a in acts]
        d.act(spec, mats[0], feed_forward=ff)  # (uploads the table before the loop)
        for k in range(policy_steps):
            d = js.model.control_steps(model, d, spec, mats[k], decimation, feed_forward=ff)
        runtime.synchronize()
        got = d.state_block()
        # out of place: the input object is untouched, the result the same as two steps in place
        a = js.data.JaxSimModelData.from_state_block(model, blk)
        b = js.model.control_steps(model, a, spec, acts[0], decimation, feed_forward=ff, inplace=False)
        c = js.model.control_steps(model, js.data.JaxSimModelData.from_state_block(model, blk), spec, acts[0], decimation, feed_forward=ff)
        runtime.synchronize()
        assert_same_bits(a.state_block(), blk, "inplace=False wrote its input")
        assert_same_bits(b.state_block(), c.state_block(), "inplace=False")
    finally:
        runtime.set_stream(None)
    assert np.isfinite(want).all()
    assert_same_bits(got, want, "the loop through the device against the loop through the host")


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch(models):
    model, other, box = sbc.build_model("icub", models), sbc.build_model("cartpole", models), sbc.build_model("box", models)
    dtype, N = np.float32, 5
    _, blk, data = icub_data(models, N, dtype)
    n = model.dofs()
    spec = icub_spec(model, dtype)
    A = spec.width
    acts = DeviceMatrix.from_host(np.zeros((N, A), np.float32))
    out = DeviceArray(n, N, dtype, tile=data._state.tile)
    data.act(spec, acts, out=out)
    before = out.to_host_raw()
    odata = js.data.JaxSimModelData.from_state_block(other, helpers.odata_to_block(other, models.random_data("cartpole", N, seed=1, dtype=dtype)))
    bad_calls = (
        lambda: odata.act(spec, acts, out=out),
        lambda: data.act(js.data.ActionSpec.build(model, dtype=np.float64), acts, out=out),
        lambda: data.act(spec, None, out=out),
        lambda: data.act(spec, DeviceMatrix(N, A + 1, dtype), out=out),
        lambda: data.act(spec, DeviceMatrix(N + 1, A, dtype), out=out),
        lambda: data.act(spec, DeviceMatrix(N, A, np.float64), out=out),
        lambda: data.act(spec, np.zeros((N, A + 1)), out=out),
        lambda: data.act(spec, acts, out=DeviceArray(n + 1, N, dtype, tile=out.tile)),
        lambda: data.act(spec, acts, out=out, feed_forward=DeviceArray(n, N + 1, dtype, tile=out.tile)),
        lambda: data.act(spec, acts, out=out, feed_forward=DeviceArray(n, N, np.float64, tile=out.tile)),
        lambda: js.data.ActionSpec.build(box),
    )
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # the entry points themselves
    lib, dm, odm, bdm = _lib.load(), runtime.device_model(model, dtype), runtime.device_model(other, dtype), runtime.device_model(box, dtype)
    one_j, one_p = np.array([[ref.POSITION, 0]], np.int32), np.array([[1.0, 0, 1, 1, 1, -1, 1, 1]])
    t = Table(bdm, one_j, one_p, 1)
    assert t.rc == -1 and t.handle.value is None and b"no joints" in lib.jxs_last_error()
    for change, word in (((0, 0, 4), "mode"), ((3, 1, A), "column"), ((3, 1, -2), "column"), ((2, 2 + ref.KP, np.inf), "finite"),
                         ((2, 2 + ref.SCALE, 1e39), "finite"), ((5, 2 + ref.ACTION_CLIP, -1.0), "action_clip"), ((5, 2 + ref.TORQUE_LIMIT, np.nan), "torque_limit"),
                         ((n - 1, 2 + ref.TARGET_LO, 9.0), "target_lo")):  # fmt: skip
        jj, pp = spec.joints.copy(), spec.params.copy()
        j, k, v = change
        if k < 2:
            jj[j, k] = v
        else:
            pp[j, k - 2] = v
        t = Table(dm, jj, pp, A)
        assert t.rc == -1 and t.handle.value is None and word in lib.jxs_last_error().decode() and f"joint {j} " in lib.jxs_last_error().decode(), lib.jxs_last_error()
    for bad_A in (-1, 4097):
        assert Table(dm, spec.joints, spec.params, bad_A).rc == -1 and b"outside" in lib.jxs_last_error()
    table = Table(dm, spec.joints, spec.params, A)
    assert table.rc == 0
    st = data._state.ptr
    assert env_act(dm, table, st, acts.ptr, dtype, A - 1, None, out.ptr, N) == -1 and b"act_ld" in lib.jxs_last_error()
    assert env_act(dm, table, st, acts.ptr, np.float64, A, None, out.ptr, N) == -1 and b"act_dtype" in lib.jxs_last_error()
    assert lib.jxs_env_act(dm.handle, table.handle, C.c_void_p(st), C.c_void_p(acts.ptr), 7, A, None, C.c_void_p(out.ptr), N, None) == -1
    assert env_act(dm, table, st, None, dtype, A, None, out.ptr, N) == -1 and b"null" in lib.jxs_last_error()
    assert env_act(dm, table, st, acts.ptr, dtype, A, None, out.ptr, 0) == -1
    assert env_act(odm, table, st, acts.ptr, dtype, A, None, out.ptr, N) == -1 and b"another" in lib.jxs_last_error()
    for k in range(4):  # state, actions, feed_forward, out: off their element size
        ptrs = [st, acts.ptr, out.ptr, out.ptr]
        ptrs[k] += 2
        assert env_act(dm, table, ptrs[0], ptrs[1], dtype, A, ptrs[2], ptrs[3], N) == -1 and b"aligned" in lib.jxs_last_error()
    assert_same_bits(out.to_host_raw(), before, "a refused call wrote the block")
    assert env_act(dm, table, st, acts.ptr, dtype, A, None, out.ptr, N) == 0
    assert_same_bits(out.to_host_raw(), before, "the same call, admitted")
    assert (bits(out.to_host_raw()[-1, :, N % out.tile :]) == 0).all()  # (the padding columns of the last tile are +0)
