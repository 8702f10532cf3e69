"""Per-environment operations (jxs_env_select, jxs_env_copy, jxs_env_flags; JaxSimModelData.reset_where / take / put /
env_flags) without a device: the NumPy restatement on the tiled storage against plain NumPy on untiled blocks, the shared
index functions of csrc/jxs_env_ops.h (driven over every word by the host harness) against the restatement bit for bit,
the refusals of the C ABI, and the host logic of the Python layer."""

import ctypes as C

import numpy as np
import pytest

import env_ops_emul as emul
import env_ops_ref as ref
from env_cpu_support import Foreign, assert_same_bits, bits, lib, refused, stub_data  # noqa: F401  (lib: a fixture)
from jaxsim_amd import _lib, runtime
from jaxsim_amd.state import tile_block, untile_block

DTYPES = (np.float32, np.float64)
GRID = [pytest.param(rows, T, N, dt, id=f"r{rows}-T{T}-N{N}-{np.dtype(dt).name}") for rows, T, N in ref.grid() for dt in DTYPES]


FLAG_GRID = [p for p in GRID if p.values[0] >= 5]  # (a block of one row holds no quaternion)


def masks_of(N, rng):
    out = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "alternating": np.arange(N) % 2 == 0, "random": rng.random(N) < 0.3}
    last = np.zeros(N, bool)
    last[N - 1] = True  # (a single environment, in the partial last tile where there is one)
    out["last"] = last
    return out


def tiled_random(rng, rows, N, T, dtype):
    """Random bit patterns in EVERY word of the storage, padding included."""
    return ref.random_bits(rng, ref.storage_words(rows, N, T), dtype)


def untile(flat, rows, N, T):
    return untile_block(flat, rows, N, T)


def index_lists(rng, src_N, dst_N):
    """(source indices, destination indices) with distinct destinations; K <= min of the two sizes."""
    K = int(rng.integers(1, min(src_N, dst_N) + 1))
    return rng.integers(0, src_N, size=K), rng.permutation(dst_N)[:K]


# ---- the restatement against plain NumPy on untiled blocks ------------------------------------------------------
@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_restatement_of_select_is_np_where(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N)
    a, b = tiled_random(rng, rows, N, T, dtype), tiled_random(rng, rows, N, T, dtype)
    for name, mask in masks_of(N, rng).items():
        out = ref.select(mask.astype(np.uint8) * 7, a, b, rows, N, T)  # (any non-zero byte is true)
        want = np.where(mask[None, :], bits(untile(a, rows, N, T)), bits(untile(b, rows, N, T)))
        assert np.array_equal(bits(untile(out, rows, N, T)), want), name
        pad = ref.word_env(rows, N, T) >= N
        assert np.array_equal(bits(out)[pad], bits(b)[pad]), f"{name}: padding columns must hold b's words"
        assert pad.sum() == (ref.n_tiles(N, T) * T - N) * rows


@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_restatement_of_copy_is_fancy_indexing(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 1)
    for dst_T, dst_N in ((T, N), (1, N + 2), (3, 2 * N + 1)):
        src, dst = tiled_random(rng, rows, N, T, dtype), tiled_random(rng, rows, dst_N, dst_T, dtype)
        si, di = index_lists(rng, N, dst_N)
        out = ref.copy(src, N, T, si, dst, dst_N, dst_T, di, rows, len(si))
        want = bits(untile(dst, rows, dst_N, dst_T)).copy()
        want[:, di] = bits(untile(src, rows, N, T))[:, si]
        assert np.array_equal(bits(untile(out, rows, dst_N, dst_T)), want)
        pad = ref.word_env(rows, dst_N, dst_T) >= dst_N
        assert np.array_equal(bits(out)[pad], bits(dst)[pad])
        # out-of-range entries are skipped entirely
        bad_s, bad_d = np.concatenate([si, [-1, N, 0, 0]]), np.concatenate([di, [0, 0, dst_N, 2**30]])
        assert np.array_equal(bits(ref.copy(src, N, T, bad_s, dst, dst_N, dst_T, bad_d, rows, len(bad_s))), bits(out))
    # null lists mean k itself
    K = min(N, 3)
    src, dst = tiled_random(rng, rows, N, T, dtype), tiled_random(rng, rows, N + 1, 1, dtype)
    out = untile(ref.copy(src, N, T, None, dst, N + 1, 1, None, rows, K), rows, N + 1, 1)
    assert np.array_equal(bits(out)[:, :K], bits(untile(src, rows, N, T))[:, :K])
    assert np.array_equal(bits(out)[:, K:], bits(untile(dst, rows, N + 1, 1))[:, K:])


def flag_state(rng, rows, N, T, dtype, row_quat):
    """Finite random states with unit quaternions, then every kind of defect in some environment (the last one included)."""
    blk = rng.normal(size=(rows, N)).astype(dtype)
    q = rng.normal(size=(4, N))
    blk[row_quat : row_quat + 4] = (q / np.linalg.norm(q, axis=0)).astype(dtype)
    kinds = {int(e): kind for e, kind in zip(rng.permutation(N)[:5], ("nan", "inf", "norm", "nan_quat", "inf_quat"))}
    kinds.setdefault(N - 1, "nan")
    for e, kind in kinds.items():
        if kind == "nan":
            blk[rows - 1, e] = np.nan  # (the last row: never one of the quaternion's)
        elif kind == "inf":
            blk[rows - 1, e] = -np.inf
        elif kind == "norm":
            blk[row_quat : row_quat + 4, e] *= dtype(1.01)
        elif kind == "nan_quat":
            blk[row_quat + 2, e] = np.nan
        elif kind == "inf_quat":
            blk[row_quat + 1, e] = np.inf
    return blk, kinds


@pytest.mark.parametrize("rows,T,N,dtype", FLAG_GRID)
def test_restatement_of_flags_is_isfinite_and_the_norm_rule(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 2)
    row_quat = 0 if rows < 7 else 3
    blk, kinds = flag_state(rng, rows, N, T, dtype, row_quat)
    got = ref.flags(tile_block(blk, T), rows, row_quat, N, T)
    bad = ~np.isfinite(blk).all(axis=0)
    q = blk[row_quat : row_quat + 4]
    with np.errstate(all="ignore"):
        q2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        not_unit = ~np.isnan(q).any(axis=0) & ~(np.abs(q2 - dtype(1)) <= dtype(1e-8) + dtype(1e-5))
    assert np.array_equal(got & 1, bad.astype(np.uint8))
    assert np.array_equal((got >> 1) & 1, not_unit.astype(np.uint8))
    for e, kind in kinds.items():
        assert got[e] == {"nan": 1, "inf": 1, "norm": 2, "nan_quat": 1, "inf_quat": 3}[kind], (e, kind)
    assert set(np.flatnonzero(got)) == set(kinds)


# ---- the shared index functions (host harness) against the restatement, bit for bit ----------------------------------
@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_harness_select_equals_the_restatement(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 3)
    a, b = tiled_random(rng, rows, N, T, dtype), tiled_random(rng, rows, N, T, dtype)
    for name, mask in masks_of(N, rng).items():
        m = mask.astype(np.uint8) * 255
        want = ref.select(m, a, b, rows, N, T)
        assert_same_bits(emul.select(m, a, b, rows, N, T), want, name)
        b2 = b.copy()
        assert_same_bits(emul.select(m, a, b2, rows, N, T, out=b2), want, f"{name}, out == b")
        a2 = a.copy()
        assert_same_bits(emul.select(m, a2, b, rows, N, T, out=a2), want, f"{name}, out == a")
        assert_same_bits(emul.select(m, a, a, rows, N, T), a, f"{name}, a == b")
    # the mask is never read at or beyond N: a guard byte behind it would flip the padding columns
    m = np.zeros(N + 64, np.uint8)
    m[N:] = 1
    assert_same_bits(emul.select(m[:N], a, b, rows, N, T), b, "all false")


@pytest.mark.parametrize("rows,T,N,dtype", GRID)
def test_harness_copy_equals_the_restatement(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 4)
    # (source tiling, destination tiling): the same, two different ones, tile 1 (environment-major) on either side
    for src_T, dst_T, dst_N in ((T, T, N), (T, 1, N + 2), (1, T, N), (T, 3, 2 * N + 1), (1, 1, N + 1)):
        src, dst = tiled_random(rng, rows, N, src_T, dtype), tiled_random(rng, rows, dst_N, dst_T, dtype)
        si, di = index_lists(rng, N, dst_N)
        assert_same_bits(emul.copy(src, N, src_T, si, dst, dst_N, dst_T, di, rows, len(si)),
                         ref.copy(src, N, src_T, si, dst, dst_N, dst_T, di, rows, len(si)), (src_T, dst_T))  # fmt: skip
        # out-of-range indices in the list: the destination is untouched for them
        bad_s = np.array([-1, N, 2**30, 0, 0, 0, -(2**31)])
        bad_d = np.array([0, 0, 0, -1, dst_N, 2**30, 0])
        assert_same_bits(emul.copy(src, N, src_T, bad_s, dst, dst_N, dst_T, bad_d, rows, len(bad_s)), dst, "only bad entries")
        mix_s, mix_d = np.concatenate([bad_s, si]), np.concatenate([bad_d, di])
        assert_same_bits(emul.copy(src, N, src_T, mix_s, dst, dst_N, dst_T, mix_d, rows, len(mix_s)),
                         ref.copy(src, N, src_T, mix_s, dst, dst_N, dst_T, mix_d, rows, len(mix_s)), "mixed")  # fmt: skip
        K = min(N, dst_N)
        assert_same_bits(emul.copy(src, N, src_T, None, dst, dst_N, dst_T, None, rows, K),
                         ref.copy(src, N, src_T, None, dst, dst_N, dst_T, None, rows, K), "null lists")  # fmt: skip
        # a null list longer than a block: the entries beyond it are skipped like any other bad index
        assert_same_bits(emul.copy(src, N, src_T, None, dst, dst_N, dst_T, None, rows, max(N, dst_N) + 3),
                         ref.copy(src, N, src_T, None, dst, dst_N, dst_T, None, rows, max(N, dst_N) + 3), "long null lists")  # fmt: skip


@pytest.mark.parametrize("rows,T,N,dtype", FLAG_GRID)
def test_harness_flags_equal_the_restatement(rows, T, N, dtype):
    rng = np.random.default_rng(rows * 1000 + N + 5)
    row_quat = 0 if rows < 7 else 3
    blk, _ = flag_state(rng, rows, N, T, dtype, row_quat)
    st = tile_block(blk, T)
    st[ref.word_env(rows, N, T) >= N] = np.nan  # (padding columns are never reported, whatever they hold)
    assert np.array_equal(emul.flags(st, rows, row_quat, N, T), ref.flags(st, rows, row_quat, N, T))
    # random bit patterns: every environment holds some NaN or huge value; the rules must still agree
    st = tiled_random(rng, rows, N, T, dtype)
    assert np.array_equal(emul.flags(st, rows, row_quat, N, T), ref.flags(st, rows, row_quat, N, T))


def test_access_width_follows_the_tile_span_and_the_addresses():
    assert emul.access_bytes(0x7F0000000000, 155, 2, 4) == 8  # the humanoid's fp32 tile: 1240 bytes, not a multiple of 16
    assert emul.access_bytes(0x7F0000000000, 155, 2, 8) == 16  # its fp64 tile: 2480 bytes
    assert emul.access_bytes(0x7F0000000008, 155, 2, 8) == 8  # (an address off the 16-byte grid)
    assert emul.access_bytes(0x7F0000000000, 5, 32, 4) == 16
    assert emul.access_bytes(0x7F0000000004, 5, 32, 4) == 4
    assert emul.access_bytes(0x7F0000000000, 1, 1, 4) == 4  # environment-major, one row
    assert emul.access_bytes(0x7F0000000000, 3, 1, 8) == 8
    # offsets are 64-bit: the last word of a block of 2^31 - 1 environments of the humanoid
    rows, T, N = 155, 2, 2**31 - 1
    assert emul.lib().jxs_emul_env_block_words(rows, N, T) == -(-N // T) * rows * T > 2**31
    assert emul.lib().jxs_emul_env_word_of(N - 1, rows - 1, rows, T) == int(ref.word_index(N - 1, rows - 1, rows, T))


# The rule of jxs_env::env_shift_for, from which the expected values below are derived (not measured): the shift starts at
# tile_shift and never passes max(tile_shift, 5); with a knob it grows until 2^shift >= knob, without one while
# N >> (shift + 1) >= 8192, that is while waves of twice as many environments would still number 8192.
@pytest.mark.parametrize("want,tile_shift,N,expected", [
    (0, 1, 1024, 1), (0, 1, 32767, 1), (0, 1, 32768, 2), (0, 1, 65536, 3), (0, 1, 2**20, 5), (0, 4, 65536, 4), (0, 4, 2**19, 5), (0, 6, 2**30, 6),
    (3, 1, None, 2), (1, 1, None, 1), (64, 1, None, 5), (8, 4, None, 4),
])  # fmt: skip
def test_environments_per_wave_follow_the_batch_size_or_the_knob(want, tile_shift, N, expected):
    for n in (1, 1024, 65536, 2**20, 2**31 - 1) if N is None else (N,):  # (a knob decides whatever the batch size)
        assert emul.env_shift_for(n, tile_shift, want) == expected, n


def test_environments_per_wave_stay_between_a_tile_and_the_larger_of_a_tile_and_32():
    for tile_shift in range(7):
        for want in (0, 1, 2, 5, 32, 33, 1000):
            for N in (1, 2, 63, 8191, 8192, 16383, 16384, 2**15 + 1, 2**17, 2**18 - 1, 2**19, 2**24, 2**30, 2**31 - 1):
                assert tile_shift <= emul.env_shift_for(N, tile_shift, want) <= max(tile_shift, 5), (N, tile_shift, want)


# ---- the C ABI refuses bad arguments without a device ---------------------------------------------------------------
def test_cabi_exports_and_refusals(lib):
    for name in ("jxs_env_select", "jxs_env_copy", "jxs_env_flags"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused before a launch)
    # jxs_env_select(mask, a, b, out, rows, N, tile, dtype, stream)
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        refused(lib, lib.jxs_env_select(*args, 5, 3, 2, _lib.JXS_F32, None), "null")
    for rows, N, tile in ((0, 3, 2), (-1, 3, 2), (5, 0, 2), (5, -3, 2), (5, 3, 0), (5, 3, -2)):
        refused(lib, lib.jxs_env_select(p, p, p, p, rows, N, tile, _lib.JXS_F32, None), "positive")
    refused(lib, lib.jxs_env_select(p, p, p, p, 5, 3, 2, 7, None), "dtype")
    # jxs_env_copy(src, src_N, src_tile, src_idx, dst, dst_N, dst_tile, dst_idx, rows, K, dtype, stream)
    refused(lib, lib.jxs_env_copy(None, 3, 2, None, p, 3, 2, None, 5, 1, _lib.JXS_F32, None), "null")
    refused(lib, lib.jxs_env_copy(p, 3, 2, None, None, 3, 2, None, 5, 1, _lib.JXS_F32, None), "null")
    good = dict(src_N=3, src_tile=2, dst_N=3, dst_tile=2, rows=5, K=1)
    for name in good:
        for bad in (0, -1):
            a = dict(good, **{name: bad})
            rc = lib.jxs_env_copy(p, a["src_N"], a["src_tile"], None, p, a["dst_N"], a["dst_tile"], None, a["rows"], a["K"], _lib.JXS_F64, None)
            refused(lib, rc, "positive")
    refused(lib, lib.jxs_env_copy(p, 3, 2, None, p, 3, 2, None, 5, 1, -1, None), "dtype")
    # jxs_env_flags(model, state, N, out_flags, stream): a model cannot exist without a device
    refused(lib, lib.jxs_env_flags(None, p, 3, p, None), "null")
    refused(lib, lib.jxs_env_flags(p, None, 3, p, None), "null")
    refused(lib, lib.jxs_env_flags(p, p, 3, None, None), "null")
    for N in (0, -1):
        refused(lib, lib.jxs_env_flags(p, p, N, p, None), "positive")  # (N is checked before the model is looked at)


# ---- host logic of the Python layer ---------------------------------------------------------------------------------
def test_host_masks_are_normalised_or_refused():
    assert np.array_equal(runtime.host_mask([True, False, True], 3), np.array([1, 0, 1], np.uint8))
    assert np.array_equal(runtime.host_mask(np.array([0, 2, 255], np.uint8), 3), np.array([0, 1, 1], np.uint8))
    assert np.array_equal(runtime.host_mask(np.array([0, -1], np.int64), 2), np.array([0, 1], np.uint8))
    assert np.array_equal(runtime.host_mask(True, 1), np.array([1], np.uint8))  # (an unbatched data object)
    for bad, n in (([True, False], 3), (np.zeros((2, 2), bool), 4), (np.zeros(3), 3), (["a", "b"], 2), (True, 2), ([], 1)):
        with pytest.raises(ValueError):
            runtime.host_mask(bad, n)


def test_host_indices_are_checked():
    assert runtime.host_indices([2, 0, 1], 3, unique=True).dtype == np.int32
    assert np.array_equal(runtime.host_indices(np.array([1, 1]), 3, unique=False), [1, 1])
    assert np.array_equal(runtime.host_indices(0, 1, unique=True), [0])
    for bad, kw in ((np.array([1, 1]), dict(unique=True)), ([0, 3], dict(unique=False)), ([-1], dict(unique=False)),
                    ([0.0, 1.0], dict(unique=False)), ([], dict(unique=False)), (np.zeros((2, 2), int), dict(unique=False)),
                    ([2**31], dict(unique=False))):  # fmt: skip
        with pytest.raises(ValueError):
            runtime.host_indices(bad, 3, **kw)


def test_foreign_device_arrays_are_used_as_they_are_or_refused():
    keep, ptr = runtime.as_device_mask(Foreign((5,), "|u1", ptr=0x2000), 5)
    assert ptr == 0x2000 and isinstance(keep, Foreign)
    assert runtime.as_device_mask(Foreign((5,), "|b1", ptr=0x3000, strides=(1,)), 5)[1] == 0x3000
    _, ptr, K, host = runtime.as_device_indices(Foreign((4,), "<i4", ptr=0x4000, strides=(4,)), 9, unique=True)
    assert (ptr, K, host) == (0x4000, 4, None)
    for bad in (Foreign((4,), "|u1"), Foreign((5, 1), "|u1"), Foreign((5,), "<i4"), Foreign((5,), "<f4"), Foreign((5,), "|i1"),
                Foreign((5,), "|u1", strides=(2,)), Foreign((5,), "|u1", ptr=0)):  # fmt: skip
        with pytest.raises(ValueError):
            runtime.as_device_mask(bad, 5)
    for bad in (Foreign((4,), "<i8"), Foreign((4,), "|u1"), Foreign((4,), "<u4"), Foreign((2, 2), "<i4"), Foreign((4,), "<i4", strides=(8,)),
                Foreign((0,), "<i4")):  # fmt: skip
        with pytest.raises(ValueError):
            runtime.as_device_indices(bad, 9, unique=True)


def test_mismatched_arguments_are_refused_on_the_host(models):
    icub, cart = models("icub"), models("cartpole")
    data = stub_data(icub, 6, np.float32)
    mask = np.zeros(6, bool)
    for fresh in (stub_data(cart, 6, np.float32), stub_data(icub, 6, np.float64), stub_data(icub, 5, np.float32),
                  stub_data(icub, 6, np.float32, tile=4), None, np.zeros(3)):  # fmt: skip
        with pytest.raises(ValueError):
            data.reset_where(mask, fresh)
        with pytest.raises(ValueError):
            data.reset_where(mask, fresh, inplace=True)
    fresh = stub_data(icub, 6, np.float32)
    for bad in (np.zeros(5, bool), np.zeros(6), Foreign((6,), "<f4"), Foreign((7,), "|u1"), "no mask"):
        with pytest.raises(ValueError):
            data.reset_where(bad, fresh)
    two = stub_data(icub, 2, np.float32)
    for idx in ([0, 0], [0, 6], [-1, 2], [0.0, 1.0], Foreign((2,), "<i8")):
        with pytest.raises(ValueError):
            data.put(idx, two)
    for other in (stub_data(cart, 2, np.float32), stub_data(icub, 2, np.float64), stub_data(icub, 3, np.float32)):
        with pytest.raises(ValueError):
            data.put(Foreign((2,), "<i4"), other)  # (device indices: the refusal is about `other`, before any launch)
    for idx in ([6], [-1], [0.5], []):
        with pytest.raises(ValueError):
            data.take(idx)
