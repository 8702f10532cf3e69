"""The random reset on the device: jxs_env_randomize on guarded raw blocks against the contract the host emulation is
held to (tests/test_env_random_cpu.py) and against the emulation itself, bit for bit where no sine or cosine is involved;
the Python layer (mask forms, agreement with the select path, shards, the episode loop, refusals)."""

import ctypes as C

import numpy as np
import pytest

import env_ops_ref as eref
import env_random_emul as emul
import env_random_ref as ref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import step_bitwise_cases as sbc
from env_cpu_support import check_contract
from env_gpu_support import CONTACT, DTYPES, MODELS, Guarded, assert_same_bits, upload_flat
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceMask
from jaxsim_amd.state import StateLayout

pytestmark = pytest.mark.gpu

SEED, DRAW, FIRST = 0xC0FFEE123456789, 0x1234567800000009, 70000


def masks_of(N):
    last = np.zeros(N, np.uint8)
    last[N - 1] = 1  # (a single environment, in the partial last tile where there is one)
    return {"none": np.zeros(N, np.uint8), "all": np.full(N, 3, np.uint8), "alternating": (np.arange(N) % 2 == 0).astype(np.uint8), "last": last}


def env_randomize(dm, mask, state_ptr, N, bounds, seed, draw, first_env, repr_):
    return _lib.load().jxs_env_randomize(dm.handle, None if mask is None else C.c_void_p(mask.ptr), C.c_void_p(state_ptr), N, C.c_void_p(bounds.ptr),
                                         seed, draw, first_env, repr_, runtime._sp())  # fmt: skip


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("key", MODELS)
def test_env_randomize_keeps_the_contract_of_the_emulation(models, key, dtype):
    model = sbc.build_model(key, models)
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    n, n_points, floating = lay.n_joints, lay.n_points, bool(model.floating_base())
    assert (dm.layout.n_rows, dm.layout.n_joints) == (lay.n_rows, n) and ref.n_rows(n, n_points) == lay.n_rows
    rng = np.random.default_rng(lay.n_rows)
    bounds_h = ref.default_bounds(n, dtype, rng)
    bounds = upload_flat(bounds_h)
    u = eref.bits_dtype(dtype)
    for N in sorted({1, T, 2 * T + 1}):
        before = eref.random_bits(rng, eref.storage_words(lay.n_rows, N, T), dtype)
        for mname, mask_h in masks_of(N).items():
            mask = upload_flat(mask_h)
            for repr_ in (ref.MIXED, ref.BODY, ref.INERTIAL):
                what = f"N={N} mask={mname} repr={repr_}"
                dst = Guarded(before)
                assert env_randomize(dm, mask, dst.ptr, N, bounds, SEED, DRAW, FIRST, repr_) == 0, _lib.load().jxs_last_error()
                got = dst.block()  # (checks the guards)
                check_contract(got, before, mask_h, n, n_points, N, T, bounds_h, SEED, DRAW, FIRST, floating, repr_, what)
                want = emul.randomize(before, mask_h, n, n_points, N, T, bounds_h, SEED, DRAW, FIRST, floating, repr_)
                bw = np.broadcast_to(ref.Rows(n, n_points).bitwise(floating, repr_)[None, :, None], (eref.n_tiles(N, T), lay.n_rows, T)).reshape(-1)
                differ = got.view(u)[bw] != want.view(u)[bw]
                assert not differ.any(), f"{what}: {int(differ.sum())} words of the uniform / zero rows differ from the emulation"
        # a null mask names every environment
        dst = Guarded(before)
        assert env_randomize(dm, None, dst.ptr, N, bounds, SEED, DRAW, FIRST, ref.MIXED) == 0
        check_contract(dst.block(), before, None, n, n_points, N, T, bounds_h, SEED, DRAW, FIRST, floating, ref.MIXED, f"N={N} null mask")


@pytest.mark.parametrize("key", ["icub", "quadruped_rigid"])
def test_the_mask_is_not_read_at_or_beyond_n(models, key):
    """The N mask bytes lie inside a larger buffer whose bytes before and behind them are all non-zero, and the last tile
    is partly padding: a kernel that read a mask byte of a padding column would find it set and write that column."""
    model, dtype = sbc.build_model(key, models), np.float32
    dm = runtime.device_model(model, dtype)
    lay, T = StateLayout.of(model), dm.layout.tile
    n, n_points, floating = lay.n_joints, lay.n_points, bool(model.floating_base())
    assert T > 1
    rng = np.random.default_rng(7)
    bounds_h = ref.default_bounds(n, dtype, rng)
    bounds = upload_flat(bounds_h)
    for N in (1, T + 1, 2 * T + 1):  # (N % T = 1: T - 1 padding columns in the last tile)
        before = eref.random_bits(rng, eref.storage_words(lay.n_rows, N, T), dtype)
        for mname, mask_h in masks_of(N).items():
            padded = np.full(64 + N + 64, 0xFF, np.uint8)
            padded[64 : 64 + N] = mask_h
            buf = upload_flat(padded)
            dst = Guarded(before)
            rc = _lib.load().jxs_env_randomize(dm.handle, C.c_void_p(buf.ptr + 64), C.c_void_p(dst.ptr), N, C.c_void_p(bounds.ptr), SEED, DRAW, FIRST,
                                               ref.BODY, runtime._sp())  # fmt: skip
            assert rc == 0, _lib.load().jxs_last_error()
            check_contract(dst.block(), before, mask_h, n, n_points, N, T, bounds_h, SEED, DRAW, FIRST, floating, ref.BODY, f"N={N} mask={mname}")


def drawn_block(model, dist, N, **kw):
    return js.data.random_model_data_device(model, batch_size=N, dist=dist, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_mask_forms_and_agreement_with_the_select_path(models, dtype):
    model = sbc.build_model("icub", models)
    T = runtime.device_model(model, dtype).layout.tile
    N = 3 * T + 1
    lay = StateLayout.of(model)
    dist = js.data.RandomStateDistribution.build(model, dtype=dtype, velocity_representation=ja.VelRepr.Body, **CONTACT)
    blk = helpers.odata_to_block(model, models.random_data("icub", N, seed=41, dtype=dtype))
    blk[lay.row_sd, [1, N - 1]] = np.nan
    make = js.data.JaxSimModelData.from_state_block
    fresh = drawn_block(model, dist, N, seed=5, draw=9)
    assert fresh.batch_size == N and fresh.dtype == dtype and fresh.velocity_representation == ja.VelRepr.Body
    fresh_h = fresh.state_block()
    assert np.isfinite(fresh_h).all() and not fresh.nonfinite_mask().any() and not (fresh.env_flags().to_host() & 2).any()
    assert (fresh_h[lay.row_m :] == 0).all()
    # mask=None: every environment; the flags of a block as they are; a host bool array
    data = make(model, blk)
    assert_same_bits(data.reset_random_where(None, dist, seed=5, draw=9).state_block(), fresh_h, "mask=None")
    flags = data.env_flags()
    assert isinstance(flags, DeviceMask)
    flagged = np.zeros(N, bool)
    flagged[[1, N - 1]] = True
    assert_same_bits(data.reset_random_where(flags, dist, seed=5, draw=9).state_block(), np.where(flagged[None, :], fresh_h, blk), "env_flags()")
    host = np.arange(N) % 3 == 0
    want = np.where(host[None, :], fresh_h, blk)
    out = data.reset_random_where(host, dist, seed=5, draw=9)
    assert out is not data and out.velocity_representation == data.velocity_representation
    assert_same_bits(out.state_block(), want, "host mask, out of place")
    assert_same_bits(data.state_block(), blk, "the functional reset wrote its input")
    # the select path gives the same bits, in place and out of place
    assert_same_bits(data.reset_where(host, fresh).state_block(), want, "reset_where, out of place")
    a, b = make(model, blk), make(model, blk)
    np.testing.assert_array_equal(a.joint_positions, blk[lay.row_s : lay.row_s + lay.n_joints].T)  # (fills the host cache)
    assert a.reset_random_where(host, dist, seed=5, draw=9, inplace=True) is a
    assert b.reset_where(host, fresh, inplace=True) is b
    assert_same_bits(a.state_block(), b.state_block(), "in place")
    assert_same_bits(a.state_block(), want, "in place")
    np.testing.assert_array_equal(a.joint_positions[0], want[lay.row_s : lay.row_s + lay.n_joints, 0])  # (a stale cache shows here)
    # another draw is another state; the joint positions of environment 0 are those of the host function
    assert not np.array_equal(drawn_block(model, dist, N, seed=5, draw=10).state_block(), fresh_h)
    if dtype == np.float64:
        s = js.joint.random_joint_positions(model, seed=5, draw=9)
        assert s.tobytes() == np.ascontiguousarray(fresh_h[lay.row_s : lay.row_s + lay.n_joints, 0]).tobytes()


@pytest.mark.parametrize("key", ["icub", "cartpole"])
def test_two_shards_draw_what_one_batch_draws(models, key):
    model = sbc.build_model(key, models)
    dist = js.data.RandomStateDistribution.build(model, dtype=np.float32)
    N = 10
    whole = drawn_block(model, dist, N, seed=3, draw=4, first_env=100).state_block()
    lo = drawn_block(model, dist, N // 2, seed=3, draw=4, first_env=100).state_block()
    hi = drawn_block(model, dist, N // 2, seed=3, draw=4, first_env=100 + N // 2).state_block()
    assert_same_bits(np.concatenate([lo, hi], axis=1), whole, "two shards")
    built = js.data.random_model_data_device(model, batch_size=N, seed=3, draw=4, first_env=100)  # (builds its own distribution)
    assert_same_bits(built.state_block(), whole, "without dist")
    if not model.floating_base():
        lay = StateLayout.of(model)
        assert (whole[lay.row_vlin : lay.row_vlin + 6].view(np.uint32) == 0).all()


def test_random_resets_inside_a_stepping_loop(models):
    model = sbc.build_model("icub", models)
    N, dtype = 6, np.float32
    lay = StateLayout.of(model)
    blk = helpers.odata_to_block(model, models.random_data("icub", N, seed=41, dtype=dtype))
    blk[lay.row_sd + 3, 4] = np.nan
    dist = js.data.RandomStateDistribution.build(model, dtype=dtype, **CONTACT)
    make = js.data.JaxSimModelData.from_state_block
    a, b = make(model, blk), make(model, blk)
    n_resets = 0
    for k in range(20):
        a = js.model.step(model, a, inplace=True)
        flags = a.env_flags()
        a.reset_random_where(flags, dist, draw=k, inplace=True)
        b = js.model.step(model, b, inplace=True)
        flags_b = b.env_flags()
        b.reset_where(flags_b, js.data.random_model_data_device(model, batch_size=N, dist=dist, draw=k), inplace=True)
        n_resets += int((flags.to_host() != 0).sum())
    assert n_resets >= 1  # (the poisoned environment was flagged and restarted)
    assert not a.env_flags().to_host().any() and not a.nonfinite_mask().any()
    assert_same_bits(a.state_block(), b.state_block(), "the loop with a fresh block per reset")


def test_refusals_happen_before_any_launch(models):
    model, other = sbc.build_model("icub", models), sbc.build_model("cartpole", models)
    dtype, N = np.float32, 5
    dist = js.data.RandomStateDistribution.build(model, dtype=dtype)
    data = js.data.random_model_data_device(model, batch_size=N, dist=dist)
    before = data.state_block()
    for bad in (js.data.RandomStateDistribution.build(other, dtype=dtype), js.data.RandomStateDistribution.build(model, dtype=np.float64), "dist"):
        with pytest.raises(ValueError):
            data.reset_random_where(None, bad, inplace=True)
    for mask in (np.ones(N + 1, bool), np.ones(N - 1, bool), np.ones(N, np.float32), DeviceMask(N + 1, zero=True)):
        with pytest.raises(ValueError):
            data.reset_random_where(mask, dist, inplace=True)
    for kw in (dict(first_env=2**32 - N + 1), dict(first_env=-1), dict(seed=2**64), dict(draw=-1)):
        with pytest.raises(ValueError):
            data.reset_random_where(None, dist, inplace=True, **kw)
    with pytest.raises(ValueError):
        js.data.random_model_data_device(model, batch_size=N, dist=dist, base_pos_bounds=(0, 1))
    # the entry point itself
    lib, dm = _lib.load(), runtime.device_model(model, dtype)
    st, bd = C.c_void_p(data._state.ptr), C.c_void_p(dist.bounds_ptr)
    assert lib.jxs_env_randomize(dm.handle, None, st, N, bd, 0, 0, 2**32 - N + 1, 2, None) == -1 and b"first_env" in lib.jxs_last_error()
    assert lib.jxs_env_randomize(dm.handle, None, st, N, bd, 0, 0, -1, 2, None) == -1
    assert lib.jxs_env_randomize(dm.handle, None, st, 0, bd, 0, 0, 0, 2, None) == -1
    assert lib.jxs_env_randomize(dm.handle, None, st, N, bd, 0, 0, 0, 3, None) == -1 and b"representation" in lib.jxs_last_error()
    assert lib.jxs_env_randomize(dm.handle, None, st, N, None, 0, 0, 0, 2, None) == -1
    assert lib.jxs_env_randomize(dm.handle, None, None, N, bd, 0, 0, 0, 2, None) == -1
    assert lib.jxs_env_randomize(None, None, st, N, bd, 0, 0, 0, 2, None) == -1 and b"null" in lib.jxs_last_error()
    assert lib.jxs_env_randomize(dm.handle, None, C.c_void_p(data._state.ptr + 2), N, bd, 0, 0, 0, 2, None) == -1
    assert_same_bits(data.state_block(), before, "a refused call wrote the block")
    assert lib.jxs_env_randomize(dm.handle, None, st, N, bd, 0, 0, 2**32 - N, 2, None) == 0  # (the last admissible shard)
    data._invalidate_caches()
    last = js.data.random_model_data_device(model, batch_size=N, dist=dist, first_env=2**32 - N)
    assert_same_bits(data.state_block(), last.state_block(), "the last admissible shard")
    assert not np.array_equal(last.state_block(), before)
