"""Per-environment operations on the device: jxs_env_select / jxs_env_copy on raw blocks against the NumPy restatement
on the tiled storage (tests/env_ops_ref.py), bit for bit and padding included; jxs_env_flags against the restatement and
against jxs_validate_state; resets inside a stepping loop against the same launches from a block the host built."""

import ctypes as C

import numpy as np
import pytest

import env_ops_ref as ref
import helpers
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from env_gpu_support import DTYPES, Guarded, assert_same_bits
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceArray, DeviceIndices, DeviceMask
from jaxsim_amd.state import StateLayout, tile_block

pytestmark = pytest.mark.gpu

GRID = [pytest.param(rows, T, N, dt, id=f"r{rows}-T{T}-N{N}-{np.dtype(dt).name}") for rows, T, N in ref.grid() for dt in DTYPES]


def upload_raw(flat, rows, N, T) -> DeviceArray:
    """A device block holding exactly these storage words (random bits in the padding columns too)."""
    out = DeviceArray(rows, N, flat.dtype, tile=T)
    assert out.nbytes == flat.nbytes
    _lib.check(_lib.load().jxs_memcpy_h2d(C.c_void_p(out.ptr), flat.ctypes.data_as(C.c_void_p), flat.nbytes, None), "h2d")
    return out


def masks_of(N):
    last = np.zeros(N, bool)
    last[N - 1] = True  # (a single environment, in the partial last tile where there is one)
    return {"none": np.zeros(N, bool), "all": np.ones(N, bool), "alternating": np.arange(N) % 2 == 0, "last": last}


def env_select(mask: DeviceMask, a, b, out, rows, N, T, dtype):
    _lib.check(_lib.load().jxs_env_select(C.c_void_p(mask.ptr), C.c_void_p(a.ptr), C.c_void_p(b.ptr), C.c_void_p(out.ptr), rows, N, T,
                                          _lib.dtype_code(dtype), runtime._sp()), "jxs_env_select")  # fmt: skip


def check_select(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 10)
    nw = ref.storage_words(rows, N, T)
    a_h, b_h = ref.random_bits(rng, nw, dtype), ref.random_bits(rng, nw, dtype)
    for name, mask in masks_of(N).items():
        m_h = mask.astype(np.uint8) * 3  # (any non-zero byte is true)
        want = ref.select(m_h, a_h, b_h, rows, N, T)
        m = DeviceMask(N)
        _lib.check(_lib.load().jxs_memcpy_h2d(C.c_void_p(m.ptr), m_h.ctypes.data_as(C.c_void_p), N, None), "h2d")
        a, b = upload_raw(a_h, rows, N, T), upload_raw(b_h, rows, N, T)
        out = upload_raw(ref.random_bits(rng, nw, dtype), rows, N, T)
        env_select(m, a, b, out, rows, N, T, dtype)
        assert_same_bits(out.to_host_raw(), want, f"{name}, out of place")
        assert_same_bits(a.to_host_raw(), a_h, f"{name}: a was written")
        assert_same_bits(b.to_host_raw(), b_h, f"{name}: b was written")
        env_select(m, a, b, b, rows, N, T, dtype)  # in place: out == b
        assert_same_bits(b.to_host_raw(), want, f"{name}, out == b")  # (all false: the block is unchanged bitwise)
        b = upload_raw(b_h, rows, N, T)
        env_select(m, a, b, a, rows, N, T, dtype)  # out == a
        assert_same_bits(a.to_host_raw(), want, f"{name}, out == a")
        env_select(m, b, b, out, rows, N, T, dtype)  # a == b
        assert_same_bits(out.to_host_raw(), b_h, f"{name}, a == b")


@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_env_select_equals_the_restatement_bitwise(rows, T, N, dtype):
    check_select(rows, T, N, dtype)


@pytest.mark.parametrize("rows,T,N,dtype", [(3, 128, 130, np.float32), (3, 128, 130, np.float64), (7, 3, 10, np.float32)])
def test_env_select_with_tiles_wider_than_a_wave_or_of_odd_width(rows, T, N, dtype):
    """Tiles of more than 64 columns read the mask per word instead of from one ballot; an odd tile span takes 4-byte accesses."""
    check_select(rows, T, N, dtype)


def env_copy(src, src_N, src_T, src_idx, dst_ptr, dst_N, dst_T, dst_idx, rows, K, dtype):
    si = None if src_idx is None else DeviceIndices.from_host(np.asarray(src_idx, dtype=np.int64))
    di = None if dst_idx is None else DeviceIndices.from_host(np.asarray(dst_idx, dtype=np.int64))
    _lib.check(_lib.load().jxs_env_copy(C.c_void_p(src.ptr), src_N, src_T, None if si is None else C.c_void_p(si.ptr), C.c_void_p(dst_ptr), dst_N, dst_T,
                                        None if di is None else C.c_void_p(di.ptr), rows, K, _lib.dtype_code(dtype), runtime._sp()), "jxs_env_copy")  # fmt: skip
    runtime.synchronize()


@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_env_copy_equals_the_restatement_and_stays_inside_its_blocks(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 11)
    # (source tiling, destination tiling): the same, two different ones, tile 1 (environment-major) on either side
    for src_T, dst_T, dst_N in ((T, T, N), (T, 1, N + 2), (1, T, N), (T, 3, 2 * N + 1)):
        src_h = ref.random_bits(rng, ref.storage_words(rows, N, src_T), dtype)
        dst_h = ref.random_bits(rng, ref.storage_words(rows, dst_N, dst_T), dtype)
        src = upload_raw(src_h, rows, N, src_T)
        K = int(rng.integers(1, min(N, dst_N) + 1))
        si, di = rng.integers(0, N, size=K), rng.permutation(dst_N)[:K]
        # out-of-range entries in the list, as source and as destination: skipped entirely
        bad_s = np.array([-1, N, 2**30, 0, 0, 0])
        bad_d = np.array([0, 0, 0, -1, dst_N, 2**30])
        for what, s, d in (("good", si, di), ("only bad", bad_s, bad_d), ("mixed", np.concatenate([bad_s, si]), np.concatenate([bad_d, di]))):
            dst = Guarded(dst_h)
            env_copy(src, N, src_T, s, dst.ptr, dst_N, dst_T, d, rows, len(s), dtype)
            want = dst_h if what == "only bad" else ref.copy(src_h, N, src_T, s, dst_h, dst_N, dst_T, d, rows, len(s))
            assert_same_bits(dst.block(), want, f"{what}, tilings {src_T} -> {dst_T}")
        # null lists mean k itself; the entries beyond the smaller block are skipped like any other bad index
        dst = Guarded(dst_h)
        K = max(N, dst_N) + 3
        env_copy(src, N, src_T, None, dst.ptr, dst_N, dst_T, None, rows, K, dtype)
        assert_same_bits(dst.block(), ref.copy(src_h, N, src_T, None, dst_h, dst_N, dst_T, None, rows, K), "null lists")
        assert_same_bits(src.to_host_raw(), src_h, "the source was written")


# ---- jxs_env_flags ---------------------------------------------------------------------------------------------------
def state_block(models, model, key, N, dtype):
    """A state block [rows, N] of a model of tests/step_bitwise_cases.py: seeded, points in contact."""
    d = models.random_data({"quadruped_rigid": "anymal"}.get(key, key), N, seed=41, dtype=dtype)
    return helpers.odata_to_block(model, d)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("key", ["icub", "cartpole", "quadruped_rigid"])
def test_env_flags_equal_the_restatement_and_the_counts_of_validate_state(models, key, dtype):
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    T, lay = dm.layout.tile, StateLayout.of(model)
    N = 3 * T + 1
    blk = state_block(models, model, key, N, dtype)
    assert np.isfinite(blk).all()
    blk[lay.row_sd + lay.n_joints - 1, 0] = np.nan  # a NaN in a joint velocity
    blk[lay.n_rows - 1, 1] = np.inf  # an infinity in a deformation row (the last row of the block)
    blk[lay.row_quat : lay.row_quat + 4, 2] *= dtype(1.01)  # a quaternion of norm 1.01
    blk[lay.row_quat + 1, N - 1] = np.nan  # a NaN quaternion, in the partial last tile
    data = js.data.JaxSimModelData.from_state_block(model, blk)
    flags = data.env_flags()
    assert isinstance(flags, DeviceMask) and flags.__cuda_array_interface__["typestr"] == "|u1"
    got = flags.to_host()
    want = np.zeros(N, np.uint8)
    want[[0, 1, N - 1]], want[2] = 1, 2
    np.testing.assert_array_equal(ref.flags(tile_block(blk, T), lay.n_rows, lay.row_quat, N, T), want)
    np.testing.assert_array_equal(got, want)
    counts = (C.c_int * 3)()
    _lib.check(_lib.load().jxs_validate_state(dm.handle, C.c_void_p(data._state.ptr), N, counts, runtime._sp()), "jxs_validate_state")
    assert (int((got & 1).sum()), int(((got >> 1) & 1).sum())) == (counts[2], counts[1]) == (3, 1)
    np.testing.assert_array_equal(data.nonfinite_mask(), (want & 1) != 0)
    # the flags are a mask: every flagged environment is reset, the others keep their words
    clean = state_block(models, model, key, N, dtype)
    fresh = js.data.JaxSimModelData.from_state_block(model, clean)
    out = data.reset_where(flags, fresh, inplace=True)
    assert out is data and not data.nonfinite_mask().any() and not data.env_flags().to_host().any()
    assert_same_bits(data.state_block(), clean, "after the reset of the flagged environments")


# ---- resets inside a stepping loop -----------------------------------------------------------------------------------
def stepped(model, data, tau, n, inplace=False):
    for _ in range(n):
        data = js.model.step(model, data, joint_force_references=tau, inplace=inplace)
    return data


@pytest.mark.parametrize("case", ["icub_f32", "cartpole_f32", "quadruped_rigid_f32"])
def test_reset_inside_a_stepping_loop_equals_the_host_built_block(models, case):
    model, blk, tau = sbc.inputs(case, models)
    N = blk.shape[1]
    fresh_blk = np.roll(blk, 1, axis=1)  # (the start states moved by one: environment 1 gets environment 0's)
    mask = np.arange(N) == 1
    make = js.data.JaxSimModelData.from_state_block
    two = stepped(model, make(model, blk), tau, 2).state_block()
    host_built = np.where(mask[None, :], fresh_blk, two)
    want = stepped(model, make(model, host_built), tau, 2).state_block()
    assert not np.array_equal(want, stepped(model, make(model, two), tau, 2).state_block())  # (the reset matters)
    fresh = make(model, fresh_blk)
    lay = StateLayout.of(model)
    # functional
    d = stepped(model, make(model, blk), tau, 2)
    r = d.reset_where(mask, fresh)
    assert r is not d and r.velocity_representation == d.velocity_representation
    assert_same_bits(d.state_block(), two, "the functional reset wrote its input")
    assert_same_bits(r.state_block(), host_built, "functional reset")
    assert_same_bits(stepped(model, r, tau, 2).state_block(), want, "steps after the functional reset")
    # in place, inside an in-place loop
    d = stepped(model, make(model, blk), tau, 2, inplace=True)
    np.testing.assert_array_equal(d.joint_positions, two[lay.row_s : lay.row_s + lay.n_joints].T)  # (fills the host cache)
    assert d.reset_where(mask, fresh, inplace=True) is d
    np.testing.assert_array_equal(d.joint_positions[1], fresh_blk[lay.row_s : lay.row_s + lay.n_joints, 1])  # (a stale cache shows here)
    assert_same_bits(stepped(model, d, tau, 2, inplace=True).state_block(), want, "steps after the in-place reset")
    assert_same_bits(fresh.state_block(), fresh_blk, "fresh was written")
    # take, then put of the same indices, restores the block; put elsewhere moves exactly those environments
    d = make(model, two)
    idx = np.array([2, 0])
    t = d.take(idx)
    assert t.batch_size == 2
    assert_same_bits(t.state_block(), two[:, idx], "take")
    assert_same_bits(d.put(idx, t).state_block(), two, "take then put")
    moved = fresh.put(idx, t)
    expect = fresh_blk.copy()
    expect[:, idx] = two[:, idx]
    assert_same_bits(moved.state_block(), expect, "put")
    assert_same_bits(fresh.state_block(), fresh_blk, "the functional put wrote its input")
    assert fresh.copy().put(DeviceIndices.from_host(idx), t, inplace=True).state_block().tobytes() == expect.tobytes()
    # device indices the host cannot check: the kernel skips the bad entry, the result's environment stays zero
    t = d.take(DeviceIndices.from_host(np.array([1, N, -1])))
    assert_same_bits(t.state_block(), np.concatenate([two[:, 1:2], np.zeros_like(two[:, :2])], axis=1), "take with bad device indices")


def test_unbatched_data_goes_through_every_operation(models):
    model = models("cartpole")
    n = model.dofs()
    data = js.data.JaxSimModelData.build(model, joint_positions=np.full(n, 0.25), dtype=np.float32)
    fresh = js.data.JaxSimModelData.build(model, joint_positions=np.full(n, -0.5), dtype=np.float32)
    assert data.batch_size == 1 and data.joint_positions.shape == (n,)
    assert not data.nonfinite_mask() and data.env_flags().to_host().tolist() == [0]
    np.testing.assert_array_equal(data.reset_where(False, fresh).joint_positions, data.joint_positions)
    np.testing.assert_array_equal(data.reset_where([True], fresh).joint_positions, fresh.joint_positions)
    t = fresh.take([0])
    assert t.batch_size == 1 and t.joint_positions.shape == (n,)
    np.testing.assert_array_equal(data.put([0], t).joint_positions, fresh.joint_positions)
    assert data.reset_where(True, fresh, inplace=True) is data
    np.testing.assert_array_equal(data.joint_positions, fresh.joint_positions)


def test_a_mask_of_another_framework_is_read_in_place(models):
    model, blk, _ = sbc.inputs("icub_f32", models)
    N = blk.shape[1]
    make = js.data.JaxSimModelData.from_state_block
    data, fresh = make(model, blk), make(model, np.ascontiguousarray(blk[:, ::-1]))
    mask = np.arange(N) % 2 == 0
    lib = _lib.load()
    raw = C.c_void_p()
    _lib.check(lib.jxs_malloc(C.byref(raw), N), "malloc")
    m_h = mask.astype(np.uint8)
    _lib.check(lib.jxs_memcpy_h2d(raw, m_h.ctypes.data_as(C.c_void_p), N, None), "h2d")
    runtime.synchronize()

    class Foreign:  # what a torch / cupy / jax bool array on the device looks like to a consumer
        def __init__(self, typestr, shape=(N,)):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (raw.value, False), "strides": None, "version": 3}

    want = data.reset_where(mask, fresh).state_block()
    assert_same_bits(want, np.where(mask[None, :], blk[:, ::-1], blk), "host mask")
    for typestr in ("|b1", "|u1"):
        assert_same_bits(data.reset_where(Foreign(typestr), fresh).state_block(), want, typestr)
    for bad in (Foreign("<f4"), Foreign("<i4"), Foreign("|u1", (N + 1,)), Foreign("|u1", (N, 1))):
        with pytest.raises(ValueError):
            data.reset_where(bad, fresh)
    runtime.synchronize()
    lib.jxs_free(raw)
