"""The contact sensors on the GPU (``-m gpu``): ``jxs_env_contacts`` on guarded raw buffers against the host harness, bit for
bit; a reset mask against zeroed timers; ``data.contact_sensors`` against ``js.contact.in_contact`` and
``collidable_point_positions``; the episode loop with the record as a source of ``evaluate`` and ``observe``; the refusals."""

import ctypes as C

import numpy as np
import pytest

import env_contact_cases as cases
import env_contact_emul as emul
import env_contact_ref as ref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import oracle
import step_bitwise_cases as sbc
from env_gpu_support import Guarded, InNaN, assert_same_bits
from jaxsim_amd import _lib, runtime
from jaxsim_amd.runtime import DeviceArray, DeviceMask, DeviceMatrix

pytestmark = pytest.mark.gpu

MODELS = ("box", "anymal", "icub", "cartpole")  # tiles 64 / 4 / 2, and a fixed base
HOST_API_SEEDS = {"anymal": 0, "icub": 0}  # chosen on the CPU with the oracle's kinematics: point_clearances() stays 1e-4 away from zero


def gpu_models(zoo):
    """Every model whose own kernels this module launches (``__graft_entry__.prebuild_specialised`` builds them, with the
    kinematics kernel ``link_kinematics`` runs).  The models of the C-ABI tests launch ``jxs_env_contacts`` alone."""
    return [zoo("box"), zoo("anymal"), zoo("icub"), sbc.build_model("quadruped_rigid", zoo)]


def terrain_of(kind):
    tr = cases.terrain(kind)
    if kind == "flat":
        return ja.FlatTerrain.build(tr.height)
    if kind == "plane":
        return ja.PlaneTerrain.build(tr.height, normal=tr.normal)
    return ja.HeightFieldTerrain.build(tr.samples, origin=tr.origin, spacing=tr.spacing, delta=tr.delta)


def raw_model(models, name, kind, dtype):
    """A device model with the terrain ``kind`` and none of its own kernels attached: these tests launch none of them."""
    return runtime.DeviceModel(helpers.with_params(models(name), terrain=terrain_of(kind)), dtype)


class InOnes:
    """A mask inside one allocation whose bytes in front of and behind it are 0xFF (``buf``, ``ptr``: set by the caller)."""

    buf = ptr = None


class Sensors:
    """A ``jxs_contact_sensors`` of a device model from an ``env_contact_ref.Table``, destroyed with the object."""

    def __init__(self, dm, tb, G=None, P=None):
        self.keep = (np.ascontiguousarray(tb.groups, np.int32), np.ascontiguousarray(tb.parent, np.int32), np.ascontiguousarray(tb.L_p, np.float64))
        g, p, L = self.keep
        self.handle = C.c_void_p()
        self.rc = _lib.load().jxs_contact_sensors_create(dm.handle, len(g) if G is None else G, g.ctypes.data_as(C.POINTER(C.c_int32)), len(p) if P is None else P,
                                                         p.ctypes.data_as(C.POINTER(C.c_int32)), L.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.handle))  # fmt: skip

    def __del__(self):
        if self.handle.value:
            _lib.load().jxs_contact_sensors_destroy(self.handle)


def env_contacts(dm, sensors, H, V, N, dt, mask, timers, out):
    vp = lambda p: None if p is None else C.c_void_p(p)  # noqa: E731
    return _lib.load().jxs_env_contacts(dm.handle, sensors.handle, vp(H), vp(V), N, dt, vp(mask), vp(timers), vp(out), runtime._sp())


def device_contacts(dm, tb, H, V, N, T, dt, timers=None, reset=None):
    """``(record storage, timer storage or None)`` of the kernel.  The link blocks and the mask lie inside NaN / non-zero
    surroundings with NaN padding columns, the record and the timers in guarded buffers; the record starts as NaN, the padding
    columns of the timers as NaN: the guards must stay, the record's padding come back zero, the timers' stay NaN."""
    dtype = H.dtype
    s = Sensors(dm, tb)
    assert s.rc == 0, _lib.load().jxs_last_error()
    bH, bV = InNaN(ref.tile_block(H, T, np.nan)), None if V is None else InNaN(ref.tile_block(V, T, np.nan))
    bm = None
    if reset is not None:  # (the surroundings of the mask are non-zero bytes, which a read beyond N would take as set)
        bm = InOnes()
        host = np.concatenate([np.full(64, 0xFF, np.uint8), np.asarray(reset, np.uint8), np.full(64, 0xFF, np.uint8)])
        bm.buf = DeviceArray(1, -(-host.size // 4), np.float32, tile=1)
        padded = np.concatenate([host, np.full(-host.size % 4, 0xFF, np.uint8)])
        _lib.check(_lib.load().jxs_memcpy_h2d(C.c_void_p(bm.buf.ptr), padded.ctypes.data_as(C.c_void_p), padded.nbytes, None), "h2d")
        bm.ptr = bm.buf.ptr + 64
    words = -(-N // T) * T
    out = Guarded(np.full(8 * tb.G * words, np.nan, dtype))
    tm = None if timers is None else Guarded(ref.tile_block(timers, T, np.nan))
    rc = env_contacts(dm, s, bH.ptr, None if bV is None else bV.ptr, N, dt, None if bm is None else bm.ptr, None if tm is None else tm.ptr, out.ptr)
    assert rc == 0, _lib.load().jxs_last_error()
    runtime.synchronize()
    return np.array(out.block()), None if tm is None else np.array(tm.block())  # (block() checks the guards)


def check_against_the_harness(dm, n_links, T, P, G, N, dtype, kind, seed=0, with_velocity=True, with_timers=True):
    tr, tb = cases.terrain(kind), cases.table(P, G, n_links)
    H, V = cases.link_blocks(n_links, N, dtype, seed=P + G + seed)
    V = V if with_velocity else None
    rng = np.random.default_rng(N)
    timers = rng.uniform(0.0, 0.4, (2 * G, N)).astype(dtype) * (rng.random((2 * G, N)) < 0.7) if with_timers else None
    reset = (rng.random(N) < 0.3).astype(np.uint8) if with_timers else None
    got, got_t = device_contacts(dm, tb, H, V, N, T, 0.002, timers, reset)
    want, want_t = emul.contacts(tr, tb, n_links, ref.tile_block(H, T), None if V is None else ref.tile_block(V, T), N, T, 0.002, reset=reset,
                                 timers=None if timers is None else ref.tile_block(timers, T))  # fmt: skip
    got, want = ref.untile_block(got, 8 * G, N, T), ref.untile_block(want, 8 * G, N, T)
    tol = None
    if kind == "field" and V is not None:
        tol = cases.SLIP_BOUND_EPS * np.finfo(dtype).eps * cases.slip_magnitude(tr, tb, H, V)
    cases.assert_records_equal(got[:, :N], want[:, :N], G, slip_tolerance=tol, what=f"record P{P} G{G} N{N} {kind}")
    assert (cases.bits(got[:, N:]) == 0).all(), "padding columns of the record are not zero"
    if with_timers:
        got_t, want_t = ref.untile_block(got_t, 2 * G, N, T), ref.untile_block(want_t, 2 * G, N, T)
        assert_same_bits(np.ascontiguousarray(got_t[:, :N]), np.ascontiguousarray(want_t[:, :N]), "timers")
        assert np.isnan(got_t[:, N:]).all(), "padding columns of the timers were written"


# ---- 1. the C-ABI contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", cases.TERRAINS)
@pytest.mark.parametrize("name", MODELS)
def test_env_contacts_keeps_the_contract_of_the_harness(models, name, kind, dtype):
    """Every (P, G, N) of tests/env_contact_cases.py on the model's own tile, synthetic link blocks, no other kernel launched:
    the record and the timers equal the harness bit for bit (SLIP_SQ on the height field within cases.SLIP_BOUND_EPS eps |pd|^2),
    guards intact, record padding zero, timer padding untouched, nothing read from a padding column or behind the mask."""
    dm = raw_model(models, name, kind, dtype)
    nL, T = models(name).number_of_links(), dm.layout.tile
    for P, G, N in cases.SHAPES:
        check_against_the_harness(dm, nL, T, P, G, N, dtype, kind)
    check_against_the_harness(dm, nL, T, 65, 4, 37, dtype, kind, with_velocity=False, with_timers=False)


@pytest.mark.parametrize("envs_per_wave", [8, 32])
def test_a_wave_of_several_tiles_and_a_partial_last_wave(models, knobs, envs_per_wave):
    """JXS_CONTACT_ENVS_PER_WAVE: waves of several tiles, the last one partly filled, a table in several chunks."""
    knobs("JXS_CONTACT_ENVS_PER_WAVE", envs_per_wave)
    for name, dtype in (("icub", np.float32), ("anymal", np.float64)):
        dm = raw_model(models, name, "field", dtype)
        for P, G, N in ((200, 4, 130), (65, 32, 37)):
            check_against_the_harness(dm, models(name).number_of_links(), dm.layout.tile, P, G, N, dtype, "field", seed=1)


# ---- 2. masked equals dense -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_reset_mask_equals_zeroed_timers(models, dtype):
    name, P, G, N = "anymal", 65, 4, 37
    dm = raw_model(models, name, "plane", dtype)
    nL, T = models(name).number_of_links(), dm.layout.tile
    tb = cases.table(P, G, nL)
    H, V = cases.link_blocks(nL, N, dtype, seed=9)
    rng = np.random.default_rng(3)
    timers = rng.uniform(0.01, 0.4, (2 * G, N)).astype(dtype)
    reset = (rng.random(N) < 0.4).astype(np.uint8)
    masked, masked_t = device_contacts(dm, tb, H, V, N, T, 0.004, timers, reset)
    zeroed = timers.copy()
    zeroed[:, reset != 0] = 0
    dense, dense_t = device_contacts(dm, tb, H, V, N, T, 0.004, zeroed, None)
    assert reset.any() and not reset.all()
    assert_same_bits(masked, dense, "record")
    assert_same_bits(ref.untile_block(masked_t, 2 * G, N, T)[:, :N].copy(), ref.untile_block(dense_t, 2 * G, N, T)[:, :N].copy(), "timers")
    unmasked, _ = device_contacts(dm, tb, H, V, N, T, 0.004, timers, None)
    assert (cases.bits(unmasked) != cases.bits(masked)).any(), "the mask changes nothing: the case shows nothing"


# ---- 3. against the host API ----------------------------------------------------------------------------------------
def host_api_case(models, name, dtype):
    d = models.random_data(name, 37, seed=HOST_API_SEEDS[name], dtype=dtype, in_contact=True)
    model = models(name)
    return model, d, helpers.odata_to_block(model, d, dtype=dtype)


def point_clearances(model, d):
    """float64 clearance of every (environment, enabled point) pair from the oracle's kinematics (flat terrain)."""
    d64 = helpers.upcast(d, model)
    p, _ = oracle.refstep.collidable_points_pos_vel(model, link_transforms=d64.link_transforms, link_velocities=d64.link_velocities)
    return np.asarray(p, np.float64)[..., 2] - model.terrain._height


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", sorted(HOST_API_SEEDS))
def test_flag_and_clearance_equal_the_host_api(models, name, dtype):
    """One group per link with enabled points: FLAG equals ``js.contact.in_contact`` for every environment and link -- after
    the float64 clearance of every (environment, point) pair was found at least 1e-4 away from zero, so that no rounding
    decides a flag --, and CLEARANCE equals min(p_z - height) of ``collidable_point_positions`` within 64 eps (1 + |p|)."""
    model, d, blk = host_api_case(models, name, dtype)
    c64 = point_clearances(model, d)
    assert np.abs(c64).min() >= 1e-4
    data = js.data.JaxSimModelData.from_state_block(model, blk)
    kdp = model.kin_dyn_parameters
    body = np.asarray(kdp.contact_body)[np.asarray(kdp.indices_of_enabled_collidable_points)]
    links = [model.link_names()[i] for i in sorted(set(body.tolist()))]
    spec = js.data.ContactSensorSpec.build(model, {ln: dict(links=[ln]) for ln in links}, dtype=dtype)
    rec = data.contact_sensors(spec).to_host()
    flags = rec[spec.rows(None, "flag")].T != 0
    want = np.asarray(js.contact.in_contact(model, data, link_names=links))
    assert flags.shape == want.shape == (37, len(links)) and np.array_equal(flags, want)
    assert want.any() and not want.all()
    p = np.asarray(js.contact.collidable_point_positions(model, data), np.float64)
    eps = np.finfo(dtype).eps
    for g, ln in enumerate(links):
        on = body == model.link_names().index(ln)
        cz = p[:, on, 2] - model.terrain._height
        k = cz.argmin(axis=1)
        bound = 64 * eps * (1 + np.linalg.norm(p[:, on][np.arange(37), k], axis=-1))
        assert (np.abs(rec[spec.rows(ln, "clearance")[0]] - cz.min(axis=1)) <= bound).all(), ln
        assert np.array_equal(rec[spec.rows(ln, "count")[0]], (cz <= 0).sum(axis=1))


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_box_below_and_above_the_ground(models, dtype):
    """The box of half height 0.05, yaw-only poses: at base height 0.02 its lowest points are 0.03 under the ground, at 0.2 they
    are 0.15 above it."""
    model = models("box")
    N = 6
    yaw = np.linspace(-3.0, 3.0, N)
    q = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1)
    pos = np.stack([np.linspace(-1, 1, N), np.linspace(1, -1, N), np.where(np.arange(N) % 2 == 0, 0.02, 0.2)], axis=1)
    d = oracle.OracleData.build(model, base_position=pos, base_quaternion=q, dtype=dtype)
    data = js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d, dtype=dtype))
    spec = js.data.ContactSensorSpec.build(model, {"box": dict(links=[model.link_names()[0]])}, dtype=dtype)
    timers = spec.new_timers(N)
    rec = data.contact_sensors(spec, timers=timers, dt=0.01).to_host()
    low = np.arange(N) % 2 == 0
    tol = 64 * np.finfo(dtype).eps * 3
    assert np.array_equal(rec[ref.FLAG] != 0, low) and (rec[ref.COUNT][low] >= 4).all() and (rec[ref.COUNT][~low] == 0).all()
    assert (np.abs(rec[ref.CLEARANCE] - np.where(low, -0.03, 0.15)) <= tol).all()
    assert (rec[ref.SLIP_SQ] == 0).all() and (rec[ref.TOUCHDOWN] == 0).all()
    assert np.array_equal(rec[ref.AIR_TIME], np.where(low, 0, dtype(0.01))) and np.array_equal(rec[ref.CONTACT_TIME], np.where(low, dtype(0.01), 0))
    assert np.array_equal(timers.to_host(), rec[[ref.AIR_TIME, ref.CONTACT_TIME]])


# ---- 4. the loop ----------------------------------------------------------------------------------------------------
def quadruped_specs(model, dtype):
    kdp = model.kin_dyn_parameters
    on = np.asarray(kdp.indices_of_enabled_collidable_points)
    body, point = np.asarray(kdp.contact_body)[on], np.asarray(kdp.contact_point, np.float64)[on]
    assert len(body) == 4 and len(set(body.tolist())) == 4
    feet = [model.link_names()[i] for i in body]
    # RigidContacts keeps a resting point AT the ground, where `c <= 0` is decided by the last bit: a foot sensor is the
    # collidable point and six points 5 mm around it, of which one is at least 2.9 mm lower whatever the link's orientation
    around = [np.zeros(3)] + [s * 0.005 * e for e in np.eye(3) for s in (-1.0, 1.0)]
    groups = {f: dict(points=[(f, tuple(p + o)) for o in around]) for f, p in zip(feet, point)}
    # the trunk has no collision shape in this model: a belly sensor of four explicit points under the base link
    groups["trunk"] = dict(points=[(model.link_names()[0], (x, y, -0.47)) for x in (-0.3, 0.3) for y in (-0.1, 0.1)])
    cs = js.data.ContactSensorSpec.build(model, groups, dtype=dtype)
    rs = js.data.RewardSpec.build(
        model,
        rewards=[("air_time", dict(term=cs.source("contacts", "flight_time", feet), weight=2.0)),
                 ("touchdowns", dict(term=cs.source("contacts", "touchdown", feet), weight=-1.0)),
                 ("slip", dict(term=cs.source("contacts", "slip_sq", feet), weight=-0.1))],
        terminations=[("trunk_on_the_ground", dict(term=cs.source("contacts", "flag", "trunk"), above=0.5))], termination_reward=-5.0, dtype=dtype)  # fmt: skip
    os_ = js.data.ObservationSpec.build(model, ["base_height", "joint_positions", cs.source("contacts", "flag", feet)], dtype=dtype)
    return cs, rs, os_, feet


def test_the_episode_loop_with_contact_sources(models):
    """20 policy steps of control_steps (``act`` + ``step``, ten times, under one action tensor: a torque action of at most
    1 N m per joint) -> link_kinematics -> contact_sensors(reset=done) -> evaluate -> reset_random_where(done) -> observe with
    nothing but device buffers, against the same loop whose record comes from the NumPy restatement on the downloaded
    kinematics (timers kept on the host): every reward, done, record and the final state and observation agree bit for bit."""
    N, dtype, iters, control_steps = 6, np.float32, 20, 10
    model = sbc.build_model("quadruped_rigid", models)
    cs, rs, os_, feet = quadruped_specs(model, dtype)
    dist = js.data.RandomStateDistribution.build(model, dtype=dtype, base_pos_bounds=((-1, -1, 0.48), (1, 1, 0.62)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3)))
    start = js.data.random_model_data_device(model, batch_size=N, dist=dist, draw=1000).state_block()
    make = js.data.JaxSimModelData.from_state_block
    tb = ref.Table(cs.groups, cs.parent, cs.L_p)
    tr = ref.Terrain(ref.FLAT, height=model.terrain._height)
    dt = control_steps * model.time_step
    aspec = js.data.ActionSpec.build(model, dtype=dtype, mode="torque", scale=1.0, action_clip=1.0)
    actions_host = np.random.default_rng(7).uniform(-1.5, 1.5, (iters, N, model.dofs())).astype(np.float32)

    def run(on_device):
        d = make(model, start)
        tile = d._state.tile
        timers = cs.new_timers(N)
        h_timers, h_done = np.zeros((cs.n_timer_rows, N), dtype), None
        done = DeviceMask(N)
        _lib.check(_lib.load().jxs_memset(C.c_void_p(done.ptr), 0, N, runtime._sp()), "jxs_memset")
        rewards, dones, records = [], [], []
        obs = DeviceMatrix(N, os_.size, dtype)
        actions = [DeviceMatrix.from_host(a) for a in actions_host]
        for k in range(iters):
            d = js.model.control_steps(model, d, aspec, actions[k], control_steps)
            kin = d.link_kinematics()
            if on_device:
                rec = d.contact_sensors(cs, kinematics=kin, timers=timers, reset=done, dt=dt)
            else:
                host_rec, h_timers = ref.sense(tr, tb, kin[0].to_host(), kin[1].to_host(), dt, h_timers, h_done)
                rec = DeviceArray.from_host(host_rec, tile=tile)
            reward, done = d.evaluate(rs, sources={"contacts": rec})
            d.reset_random_where(done, dist, draw=k, inplace=True)
            d.observe(os_, out=obs, sources={"contacts": rec})
            if not on_device:
                h_done = done.to_host()
            rewards.append(reward), dones.append(done), records.append(rec)
        runtime.synchronize()
        return (d.state_block(), obs.to_host(), [r.to_host()[:, 0] for r in rewards], [m.to_host() for m in dones], [r.to_host() for r in records],
                timers.to_host() if on_device else h_timers)  # fmt: skip

    want, got = run(False), run(True)
    recs = np.stack(want[4]).reshape(iters, cs.n_groups, 8, N)
    seen = dict(trunk=int((np.concatenate(want[3]) & 1).sum()), touchdown=int((recs[:, :4, ref.TOUCHDOWN] == 1).sum()),
                air=int((recs[:, :4, ref.AIR_TIME] > 0).sum()), slip=int((recs[:, :4, ref.SLIP_SQ] > 0).sum()))  # fmt: skip
    print("the loop saw:", seen, "of", iters * N, "environment steps")
    assert all(seen.values()) and seen["trunk"] < iters * N, f"the case must see a trunk contact, a touchdown, a flight and a slipping foot: {seen}"
    assert np.isfinite(want[0]).all()
    for k in range(iters):
        assert_same_bits(got[4][k], want[4][k], f"record of iteration {k}")
        assert np.array_equal(got[3][k], want[3][k]), f"done of iteration {k}"
        assert_same_bits(got[2][k], want[2][k], f"reward of iteration {k}")
    assert_same_bits(got[5], want[5], "timers")
    assert_same_bits(got[0], want[0], "the final state")
    assert_same_bits(got[1], want[1], "the observation behind the loop")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch(models):
    model, other = models("anymal"), models("icub")
    dtype, N = np.float32, 5
    build = js.data.ContactSensorSpec.build
    a_link = model.link_names()[0]
    for bad in (dict(g=dict(links=["no_such_link"])), dict(g=dict(points=[("no_such_link", (0, 0, 0))])), dict(g=dict(links=[])), dict(g=dict(points=[])),
                dict(g=dict(points=[(a_link, (0, np.nan, 0))])), dict(g=dict(points=[(a_link, (0, 1e39, 0))])), dict(g=dict(points=[(a_link, (0, 0))])),
                dict(g=dict(both=[])), {}, {f"g{i}": dict(points=[(a_link, (0, 0, 0))]) for i in range(33)},
                dict(g=dict(points=[(a_link, (0, 0, 0))] * 1025))):  # fmt: skip
        with pytest.raises(ValueError):
            build(model, bad, dtype=dtype)
    with pytest.raises(ValueError):
        build(model, dict(g=dict(points=[(a_link, (0, 0, 0))])), dtype=np.float16)
    spec = build(model, {"base": dict(points=[(a_link, (0.1, 0, -0.2)), (a_link, (-0.1, 0, -0.2))])}, dtype=dtype)
    with pytest.raises(ValueError):
        spec.rows("base", "no_such_field")
    with pytest.raises(ValueError):
        spec.rows("no_such_group", "flag")
    data = js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, models.random_data("anymal", N, seed=1, dtype=dtype)))
    odata = js.data.JaxSimModelData.from_state_block(other, helpers.odata_to_block(other, models.random_data("icub", N, seed=1, dtype=dtype)))
    H, V = data.link_kinematics()
    timers, out = spec.new_timers(N), DeviceArray(spec.n_rows, N, dtype, tile=H.tile, zero=True)
    data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=out)
    before = [out.to_host(), timers.to_host()]
    nL = model.number_of_links()
    bad_calls = (
        lambda: odata.contact_sensors(spec),
        lambda: data.contact_sensors(build(model, {"b": dict(points=[(a_link, (0, 0, 0))])}, dtype=np.float64), kinematics=(H, V), out=out),
        lambda: data.contact_sensors("spec", kinematics=(H, V), out=out),
        lambda: data.contact_sensors(spec, kinematics=H, out=out),
        lambda: data.contact_sensors(spec, kinematics=(V, H), out=out),
        lambda: data.contact_sensors(spec, kinematics=(DeviceArray(nL * 12, N + 1, dtype, tile=H.tile), V), out=out),
        lambda: data.contact_sensors(spec, kinematics=(H, DeviceArray(nL * 6 + 1, N, dtype, tile=H.tile)), out=out),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=DeviceArray(spec.n_timer_rows + 1, N, dtype, tile=H.tile), out=out),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=DeviceArray(spec.n_timer_rows, N, np.float64, tile=H.tile), out=out),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=DeviceArray(spec.n_rows - 1, N, dtype, tile=H.tile)),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=out, dt=-1e-3),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=out, dt=np.nan),
        lambda: data.contact_sensors(spec, kinematics=(H, V), timers=timers, out=out, reset=DeviceMask(N + 1)),
        lambda: data.link_kinematics(out=(V, H)),
        lambda: data.link_kinematics(out=H),
    )
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # the entry points themselves
    lib, dm, odm = _lib.load(), runtime.device_model(model, dtype), runtime.device_model(other, dtype)
    good = cases.table(20, 4, nL)
    import dataclasses

    def refused(tb, word, **kw):
        s = Sensors(dm, tb, **kw)
        assert s.rc == -1 and s.handle.value is None and word in lib.jxs_last_error().decode() and b"jxs_contact_sensors_create" in lib.jxs_last_error(), lib.jxs_last_error()

    refused(good, "outside", G=0), refused(good, "outside", G=33), refused(good, "outside", P=0), refused(good, "outside", P=1025)
    g = good.groups.copy()
    g[2, 1] = 0
    refused(dataclasses.replace(good, groups=g), "group 2")
    g = good.groups.copy()
    g[1, 0] -= 1
    refused(dataclasses.replace(good, groups=g), "group 1")
    g = good.groups.copy()
    g[1, 1] -= 1
    refused(dataclasses.replace(good, groups=g), f"entry {good.groups[1].sum() - 1} belongs to no group")
    p = good.parent.copy()
    p[5] = nL
    refused(dataclasses.replace(good, parent=p), "entry 5: parent link")
    L = good.L_p.copy()
    L[7, 1] = np.inf
    refused(dataclasses.replace(good, L_p=L), "entry 7: L_p")
    L[7, 1] = 1e39
    refused(dataclasses.replace(good, L_p=L), "entry 7: L_p")
    s = Sensors(dm, ref.Table(spec.groups, spec.parent, spec.L_p))
    assert s.rc == 0, lib.jxs_last_error()
    full = dict(dm_=dm, s_=s, H_=H.ptr, V_=V.ptr, N_=N, dt_=1e-3, mask=None, timers=timers.ptr, out=out.ptr)
    call = lambda **kw: (lambda a: env_contacts(a["dm_"], a["s_"], a["H_"], a["V_"], a["N_"], a["dt_"], a["mask"], a["timers"], a["out"]))({**full, **kw})  # noqa: E731
    assert call(H_=None) == -1 and b"null" in lib.jxs_last_error()
    assert call(out=None) == -1 and b"null" in lib.jxs_last_error()
    assert lib.jxs_env_contacts(dm.handle, None, C.c_void_p(H.ptr), None, N, 1e-3, None, None, C.c_void_p(out.ptr), None) == -1
    assert lib.jxs_env_contacts(None, s.handle, C.c_void_p(H.ptr), None, N, 1e-3, None, None, C.c_void_p(out.ptr), None) == -1
    assert call(N_=0) == -1
    for bad_dt in (-1e-3, np.nan, np.inf, 1e39):
        assert call(dt_=bad_dt) == -1 and b"dt" in lib.jxs_last_error()
    assert call(dm_=odm) == -1 and b"another" in lib.jxs_last_error()
    assert call(dm_=runtime.device_model(model, np.float64)) == -1 and b"another" in lib.jxs_last_error()
    for key in ("H_", "V_", "timers", "out"):
        assert call(**{key: full[key] + 2}) == -1 and b"aligned" in lib.jxs_last_error()
    runtime.synchronize()
    for got, was in zip([out.to_host(), timers.to_host()], before):
        assert_same_bits(got, was, "a refused call wrote an output")
