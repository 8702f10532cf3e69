"""The random reset on the CPU: the functions of jaxsim_amd/csrc/jxs_env_random.h, run over every word of a block by
the host harness (tests/env_random_emul.py), against the NumPy restatement written from the specification
(tests/env_random_ref.py); the host logic of the Python layer (joint sampling window, random_joint_positions, bounds)."""

import re

import numpy as np
import pytest

import env_ops_ref as eref
import env_random_emul as emul
import env_random_ref as ref
import jaxsim_amd as ja
import jaxsim_amd.api as js
from env_cpu_support import check_contract
from jaxsim_amd import _lib, robots
from jaxsim_amd.state import StateLayout

DTYPES = (np.float32, np.float64)
# (joints, collidable points): no, one and 23 joints, with and without point rows
LAYOUTS = ((0, 0), (0, 8), (1, 0), (1, 2), (23, 0), (23, 32))
TILES = (1, 2, 4, 64)
REPRS = {"inertial": ref.INERTIAL, "body": ref.BODY, "mixed": ref.MIXED}
SEED, DRAW, FIRST = 0x123456789ABCDEF, 0xFEDCBA9876543210, 1000


def masks_of(N):
    last = np.zeros(N, np.uint8)
    last[N - 1] = 1
    return {"null": None, "none": np.zeros(N, np.uint8), "all": np.full(N, 3, np.uint8), "alternating": (np.arange(N) % 2 == 0).astype(np.uint8), "last": last}


def test_philox_known_answers():
    for ctr, key, out in ref.KNOWN_ANSWERS:
        assert emul.philox(ctr, key) == out
        assert tuple(int(x) for x in ref.philox4x32_10(ctr, key)) == out


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n,n_points", LAYOUTS)
def test_emulation_equals_the_restatement(n, n_points, dtype):
    rng = np.random.default_rng(100 * n + n_points)
    rows = ref.n_rows(n, n_points)
    for T in TILES:
        for N in sorted({1, T, 2 * T + 1}):
            before = eref.random_bits(rng, eref.storage_words(rows, N, T), dtype)
            bounds = ref.default_bounds(n, dtype, rng)
            for mname, mask in masks_of(N).items():
                for rname, repr_ in REPRS.items():
                    for floating in (True, False) if rname == "mixed" else (True,):
                        got = emul.randomize(before, mask, n, n_points, N, T, bounds, SEED, DRAW, FIRST, floating, repr_)
                        check_contract(got, before, mask, n, n_points, N, T, bounds, SEED, DRAW, FIRST, floating, repr_,
                                       f"T={T} N={N} mask={mname} {rname} floating={floating}")  # fmt: skip


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_state_depends_on_seed_draw_and_global_environment_only(dtype):
    n, n_points = 3, 2
    rows = ref.n_rows(n, n_points)
    bounds = ref.default_bounds(n, dtype, np.random.default_rng(5))
    u = eref.bits_dtype(dtype)

    def drawn(N, T, first, mask=None, seed=SEED, draw=DRAW):
        st = np.zeros(eref.storage_words(rows, N, T), dtype=dtype)
        return ref.untile(emul.randomize(st, mask, n, n_points, N, T, bounds, seed, draw, first, True, ref.BODY), rows, N, T)

    whole = drawn(16, 2, 0)[:, 5:10]
    shard = drawn(5, 64, 5)
    only = np.zeros(16, np.uint8)
    only[5:10] = 1
    masked = drawn(16, 2, 0, only)
    assert (whole.view(u) == shard.view(u)).all() and (whole.view(u) == masked[:, 5:10].view(u)).all()
    assert (np.delete(masked, np.arange(5, 10), axis=1).view(u) == 0).all()
    # another draw or seed changes every sampled word of every one of 64 environments
    a = drawn(64, 4, 0)
    sampled = np.arange(rows) < 13 + 2 * n
    for other in (drawn(64, 4, 0, draw=DRAW + 1), drawn(64, 4, 0, seed=SEED + 1), drawn(64, 4, 0, draw=DRAW ^ (1 << 40)), drawn(64, 4, 0, seed=SEED ^ (1 << 40))):
        assert (a.view(u)[sampled] != other.view(u)[sampled]).all()
        assert (other.view(u)[~sampled] == 0).all()
    # first_env + N may reach 2^32 and not pass it
    st = np.zeros(eref.storage_words(rows, 2, 2), dtype=dtype)
    assert emul.randomize(st, None, n, n_points, 2, 2, bounds, 0, 0, 2**32 - 2, rc=True) == 0
    assert emul.randomize(st, None, n, n_points, 2, 2, bounds, 0, 0, 2**32 - 1, rc=True) == -2
    assert emul.randomize(st, None, n, n_points, 2, 2, bounds, 0, 0, -1, rc=True) == -2
    top = ref.untile(emul.randomize(st, None, n, n_points, 2, 2, bounds, 1, 2, 2**32 - 2), rows, 2, 2)
    want, _ = ref.sampled_block(n, n_points, bounds, 2**32 - 2 + np.arange(2), 1, 2, True, ref.MIXED)
    bw = ref.Rows(n, n_points).bitwise(True, ref.MIXED)
    assert (top.view(u)[bw] == want.view(u)[bw]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_range_and_moments(dtype):
    n, N, T = 2, 4096, 64
    rows = ref.n_rows(n, 0)
    bounds = ref.default_bounds(n, dtype, np.random.default_rng(9))
    bounds[:, 1] = 0.75  # lo == hi
    bounds[:, 6] = (0.0, 1.0)  # the value of variable 6 (joint 0, row 7) is u itself
    st = np.zeros(eref.storage_words(rows, N, T), dtype=dtype)
    blk = ref.untile(emul.randomize(st, None, n, 0, N, T, bounds, 77, 5, 0, True, ref.INERTIAL), rows, N, T)
    L = ref.Rows(n, 0)
    var_rows = np.r_[0:3, L.s : L.s + n, L.vlin : L.vlin + 6, L.sd : L.sd + n]
    var_idx = np.r_[0:3, 6 : 6 + n, 6 + n : 12 + 2 * n]
    lo, hi = bounds[0, var_idx, None], bounds[1, var_idx, None]
    assert ((blk[var_rows] >= lo) & (blk[var_rows] <= hi)).all()
    assert (blk[1] == dtype(0.75)).all()
    u = blk[7].astype(np.float64)
    assert abs(u.mean() - 0.5) <= 5 / np.sqrt(12 * N)
    counts = np.bincount(np.minimum((u * 16).astype(int), 15), minlength=16)
    assert (np.abs(counts - 256) <= 5 * np.sqrt(256 * 15 / 16)).all(), counts
    # the clamp: a value can never pass hi, also where lo + u (hi - lo) rounds up (a narrow interval far from zero)
    bounds[:, 6] = (dtype(1e6), np.nextafter(dtype(1e6), dtype(2e6)))
    blk = ref.untile(emul.randomize(st, None, n, 0, N, T, bounds, 77, 5, 0, True, ref.INERTIAL), rows, N, T)
    assert ((blk[7] >= bounds[0, 6]) & (blk[7] <= bounds[1, 6])).all()


# ---- host logic of the Python layer ------------------------------------------------------------------------------------
def test_the_joint_sampling_window_follows_the_rule_of_the_reference():
    pi, fmax = np.pi, np.finfo(float).max
    #          wide revolute   continuous      one-sided (upper)  one-sided (lower)  narrow revolute  prismatic
    s_min = [-4.0, -fmax, -np.inf, -1.0, -0.5, -7.0]
    s_max = [5.0, fmax, 1.0, np.inf, 0.25, 9.0]
    lo, hi = js.joint.random_position_window(s_min, s_max, [True, True, True, True, True, False])
    np.testing.assert_array_equal(lo, [-pi, -pi, 1.0 - 2 * pi, -1.0, -0.5, -7.0])
    np.testing.assert_array_equal(hi, [pi, pi, 1.0, -1.0 + 2 * pi, 0.25, 9.0])


def test_bounds_table_defaults_broadcasting_and_refusals():
    model = ja.JaxSimModel.build_from_model_description(robots.icub23_urdf())
    n = model.number_of_joints()
    for dtype in DTYPES:
        t = js.data.random_state_bounds(model, dtype=dtype)
        assert t.shape == (2, 12 + 2 * n) and t.dtype == dtype
        np.testing.assert_array_equal(t[:, 0:3], np.array([[-1, -1, 0.5], [1, 1, 1]], dtype=dtype))
        np.testing.assert_array_equal(t[:, 3:6], np.array([[-np.pi] * 3, [np.pi] * 3]).astype(dtype))
        lo, hi = js.joint.random_position_bounds(model, dtype=dtype)
        np.testing.assert_array_equal(t[:, 6 : 6 + n], np.stack([lo, hi]))
        np.testing.assert_array_equal(t[:, 6 + n :], np.stack([-np.ones(6 + n), np.ones(6 + n)]).astype(dtype))
    t = js.data.random_state_bounds(model, dtype=np.float64, joint_pos_bounds=(-0.1, np.full(n, 0.2)), base_vel_lin_bounds=((0, 1, 2), 3.0))
    np.testing.assert_array_equal(t[:, 6 : 6 + n], np.stack([np.full(n, -0.1), np.full(n, 0.2)]))
    np.testing.assert_array_equal(t[:, 6 + n : 9 + n], [[0, 1, 2], [3, 3, 3]])
    for bad in (dict(joint_pos_bounds=(-np.inf, 1.0)), dict(base_pos_bounds=(0.0, np.nan)), dict(joint_vel_bounds=(1.0, -1.0)),
                dict(joint_vel_bounds=(np.zeros(n + 1), 1.0)), dict(base_pos_bounds=(0.0,))):  # fmt: skip
        with pytest.raises(ValueError):
            js.data.random_state_bounds(model, dtype=np.float32, **bad)
    # a joint without a finite range: refused with a message that names the way out, instead of the reference's NaN samples
    kdp = model.kin_dyn_parameters
    saved, saved_min = kdp.position_limits_max.copy(), kdp.position_limits_min.copy()
    prismatic = kdp.joint_types.copy()
    try:
        kdp.position_limits_max[2], kdp.position_limits_min[2] = np.finfo(float).max, -np.finfo(float).max  # continuous: [-pi, pi]
        js.data.random_state_bounds(model, dtype=np.float32)
        kdp.joint_types[2] = 2  # the same limits on a prismatic joint
        with pytest.raises(ValueError, match="joint_pos_bounds"):
            js.data.random_state_bounds(model, dtype=np.float32)
        with pytest.raises(ValueError, match="joint_pos_bounds"):
            js.joint.random_joint_positions(model)
        js.data.random_state_bounds(model, dtype=np.float32, joint_pos_bounds=(-1.0, 1.0))
    finally:
        kdp.position_limits_max[:], kdp.position_limits_min[:] = saved, saved_min
        kdp.joint_types[:] = prismatic


@pytest.mark.parametrize("robot", ["icub23", "cartpole"])
def test_random_joint_positions_equal_the_emulated_environment_zero(robot):
    model = ja.JaxSimModel.build_from_model_description(getattr(robots, robot + "_urdf")())
    lay = StateLayout.of(model)
    n, n_points = lay.n_joints, lay.n_points
    bounds = js.data.random_state_bounds(model, dtype=np.float64)
    st = np.zeros(eref.storage_words(lay.n_rows, 3, 2), dtype=np.float64)
    blk = ref.untile(emul.randomize(st, None, n, n_points, 3, 2, bounds, 12345, 678, 0, model.floating_base(), ref.MIXED), lay.n_rows, 3, 2)
    s = js.joint.random_joint_positions(model, seed=12345, draw=678)
    assert s.dtype == np.float64 and s.shape == (n,)
    assert s.tobytes() == blk[lay.row_s : lay.row_s + n, 0].tobytes()
    assert not np.array_equal(s, js.joint.random_joint_positions(model))  # (seed 0, draw 0: another sample)
    names = model.joint_names()[::-2]
    part = js.joint.random_joint_positions(model, joint_names=names, seed=12345, draw=678)
    assert part.tobytes() == s[js.joint.names_to_idxs(model, joint_names=names)].tobytes()
    lo, hi = js.joint.random_position_bounds(model)
    assert ((s >= lo) & (s <= hi)).all()
    # the product's NumPy Philox against the restatement
    from jaxsim_amd import _philox

    for ctr, key, out in ref.KNOWN_ANSWERS:
        assert tuple(int(x) for x in _philox.philox4x32_10(ctr, key)) == out


def test_the_ctypes_prototype_is_the_one_of_the_header():
    """Parameter by parameter: a 64-bit seed, draw or first_env declared as a C int on the Python side would be cut to
    32 bits without any error.  (tests/test_cabi.py checks that the header, the exports and EXPORTED_SYMBOLS agree on the
    names.)"""
    import ctypes as C

    if not _lib.LIB_PATH.exists():
        import __graft_entry__

        __graft_entry__.build()
    text = re.sub(r"/\*.*?\*/", "", (_lib.LIB_PATH.parent.parent.parent / "include" / "jaxsim_amd.h").read_text(), flags=re.S)
    proto = re.search(r"int jxs_env_randomize\((.*?)\);", text, flags=re.S).group(1)
    want = []
    for param in proto.split(","):
        words = param.replace("*", " * ").split()
        if "*" in words:
            want.append(C.c_void_p)
        else:
            want.append({"int": C.c_int, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[words[-2]])
    names = [p.replace("*", " ").split()[-1] for p in proto.split(",")]
    assert names == ["model", "mask", "state", "N", "bounds", "seed", "draw", "first_env", "velocity_representation", "stream"]
    fn = _lib.load().jxs_env_randomize
    assert list(fn.argtypes) == want and fn.restype is C.c_int
    assert "jxs_env_randomize" in _lib.EXPORTED_SYMBOLS
    assert hasattr(js.data, "random_model_data_device") and hasattr(js.data.JaxSimModelData, "reset_random_where")
    assert "not provided" not in js.joint.__doc__
