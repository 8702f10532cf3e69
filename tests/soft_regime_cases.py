"""TEST INFRASTRUCTURE: the states, cases and input conditions of tests/test_soft_regimes_cpu.py (host emulation) and
tests/test_soft_regimes_gpu.py (device) -- the Hunt-Crossley law of ``point_physics`` (jaxsim_amd/csrc/jxs_core.h) branch
by branch.

The random states of the zoo leave most branches of the law to chance (of 2240 humanoid points of a parity test one
slips, none lifts off, none rests).  ``regime_states`` aims every environment at one regime -- sticking, slipping,
lift-off (the clamp ``fn = max(0, .)``), rest (``ft == 0``) or airborne with a loaded spring -- at depths from 1e-5 m
(1e-4 m in float32) to 1e-2 m, ``regimes`` restates the law's intermediate quantities per point in fp64 and classifies
them, and ``require`` asserts on the INPUTS that a case reaches every regime before anything is compared.
"""

from __future__ import annotations

import dataclasses

import numpy as np

import height_field_cases as hfc
import helpers
import jaxsim_amd as ja
import oracle
from jaxsim_amd import robots
from parity_cases import RK4_SOFT  # the softer ground of every Runge-Kutta case of the suite
from jaxsim_amd import state as st
from oracle import VelRepr
from oracle import refmath as rm

REGIMES = ("stick", "slip", "liftoff", "rest", "airborne")  # environment e aims at REGIMES[e % 5]
C_V = (0.15, 4.0, 0.5, 0.0, 1.0)  # base velocity in units of mu * v_eq, v_eq = (K / D) * sink^(1 + p - q)
C_M = (0.15, 1.0, 0.3, 0.0, 1.0)  # deformation in units of mu * sink
N_ENV, SEED = 40, 7
# (on the tilted plane one corner of a box touches per environment: 40 environments leave 2 slipping points with m . n != 0)
N_BY_MODEL = {"box": 80}
SINK_LO = {np.dtype(np.float64): -5.0, np.dtype(np.float32): -4.0}
MU0_SCALE = 0.5  # stands in for mu in the recipe of the frictionless cases
PLANE = dict(height=0.02, normal=[0.15, -0.1, 1.0])


# ---- the classifier ------------------------------------------------------------------------------------------------------
def regimes(model, d) -> dict:
    """The law's intermediate quantities per ENABLED point ([N, nc] arrays, fp64, from the oracle's point kinematics and
    penetration data), the regime masks, and the force and rate rebuilt from them (``force``, ``m_dot``: the CPU module
    checks these against ``oracle.refstep.hunt_crossley_contact_model``, so the classifier cannot drift from the oracle).

    airborne: delta <= 0 | stick: fn > 0, |ft| <= 0.8 mu fn | slip: fn > 0, |ft| >= 1.25 mu fn | liftoff: delta > 0,
    fn_raw < 0 | rest: delta > 0, |ft| == 0 (|ft| before clipping).  ``slipping`` is the law's own branch."""
    assert d.dtype == np.float64
    kdp, cp = model.kin_dyn_parameters, model.contact_params
    idx = kdp.indices_of_enabled_collidable_points
    p, v = oracle.refstep.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    m = d.tangential_deformation[:, idx]
    delta, ddelta, n = oracle.refstep.compute_penetration_data(model, p, v)
    h = model.terrain.height(p[..., 0], p[..., 1]) - p[..., 2]
    eps = np.finfo(np.float64).eps
    dp, dq = np.power(delta + eps, cp.p), np.power(delta + eps, cp.q)
    fn_raw = (cp.K * dp) * delta + (cp.D * dq) * ddelta
    fn = np.maximum(0.0, fn_raw)
    dot = lambda a, b: np.sum(a * b, axis=-1, keepdims=True)  # noqa: E731
    vt = v - dot(v, n) * n
    m_n = dot(m, n)[..., 0]
    mt = m - dot(m, n) * n
    ft0 = -((cp.K * dp)[..., None] * mt + (cp.D * dq)[..., None] * vt)
    ft = rm.safe_norm(ft0)
    contact = delta > 0
    slipping = contact & ~(dot(ft0, ft0)[..., 0] <= (cp.mu * fn) ** 2)
    # the force and the rate, from the quantities above
    ft_clip = np.where(slipping[..., None], np.minimum(cp.mu * fn, ft)[..., None] * (ft0 / (ft + eps * (ft == 0))[..., None]), ft0)
    ft_clip = np.where(contact[..., None], ft_clip, 0.0)
    md_sl = -(ft_clip + (cp.K * dp)[..., None] * mt) / (cp.D * dq)[..., None]
    md = np.where(slipping[..., None], md_sl, np.where(contact[..., None], vt - (cp.K / cp.D) * dot(m, n) * n, -(cp.K / cp.D) * m))
    return dict(
        delta=delta, fn_raw=fn_raw, fn=fn, ft=ft, h=h, m_n=m_n, m_norm=np.linalg.norm(m, axis=-1), contact=contact, slipping=slipping,
        airborne=~contact, stick=(fn > 0) & (ft <= 0.8 * cp.mu * fn), slip=(fn > 0) & (ft >= 1.25 * cp.mu * fn),
        liftoff=contact & (fn_raw < 0), rest=contact & (ft == 0), force=fn[..., None] * n + ft_clip, m_dot=md,
        position=p, velocity=v, m=m,
    )  # fmt: skip


def counts(R: dict) -> dict:
    return {k: int(R[k].sum()) for k in REGIMES}


# ---- the state recipe ----------------------------------------------------------------------------------------------------
def regime_states(model, N=N_ENV, seed=SEED, sink_lo=-5.0, dtype=np.float64, rep=VelRepr.Inertial, mu_scale=None):
    """(state, sink [N], vs [N]): small joint angles, roll and pitch, any yaw, base x, y in +-0.4; the base height puts the
    deepest enabled point ``sink = 10^U(sink_lo, -2)`` under the model's own terrain (airborne environments: 1e-4 .. 1e-2
    above it); one horizontal base velocity of c mu v_eq (lift-off: and 3 v_eq upwards), no angular or joint velocity --
    every point moves alike; deformations of cm mu sink U(0.5, 1) along a direction with a unit
    horizontal and a 0.3 U(-1, 1) vertical part.  ``model`` carries the terrain the oracle evaluates.

    v_eq = (K / D) sink^(1 + p - q) is the speed at which the damper D delta^q v balances the spring K delta^p delta at
    depth sink; for p = q it is vs = (K / D) sink, the scale of m_dot that is returned.  (With p = 0.7, q = 0.3 a velocity
    of 0.15 mu vs is sink^-0.4, 6 .. 100 times, too fast to stick: no point with m != 0 would stick.)"""
    rng = np.random.default_rng(seed)
    kdp, cp = model.kin_dyn_parameters, model.contact_params
    n, n_cp, idx = kdp.number_of_joints(), kdp.number_of_collidable_points(), kdp.indices_of_enabled_collidable_points
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape)  # noqa: E731
    s = 0.03 * u(N, n)
    quat = rm.quaternion_from_euler_xyz(np.stack([0.05 * u(N), 0.05 * u(N), 3.0 * u(N)], axis=1))
    xy = 0.4 * u(N, 2)
    target = np.arange(N) % 5
    sink = 10.0 ** rng.uniform(sink_lo, -2.0, N)
    clear = 10.0 ** rng.uniform(-4.0, -2.0, N)
    pos = np.concatenate([xy, np.zeros((N, 1))], axis=1)
    d0 = oracle.OracleData.build(model, base_position=pos, base_quaternion=quat, joint_positions=s)
    p, _ = oracle.refstep.collidable_points_pos_vel(model, link_transforms=d0.link_transforms, link_velocities=d0.link_velocities)
    h0 = (model.terrain.height(p[..., 0], p[..., 1]) - p[..., 2]).max(axis=1)
    pos[:, 2] = h0 + np.where(target == 4, clear, -sink)
    mu = cp.mu if mu_scale is None else mu_scale
    vs = (cp.K / cp.D) * sink
    v_eq = vs * sink ** (cp.p - cp.q)
    ang = rng.uniform(0.0, 2.0 * np.pi, N)
    vel = (np.take(C_V, target) * mu * v_eq)[:, None] * np.stack([np.cos(ang), np.sin(ang), np.zeros(N)], axis=1)
    vel[:, 2] += np.where(target == 2, 3.0 * v_eq, 0.0)
    nc = len(idx)
    ang_m = rng.uniform(0.0, 2.0 * np.pi, (N, nc))
    mdir = np.stack([np.cos(ang_m), np.sin(ang_m), 0.3 * u(N, nc)], axis=-1)
    m = np.zeros((N, n_cp, 3))
    m[:, idx] = (np.take(C_M, target) * mu * sink)[:, None, None] * rng.uniform(0.5, 1.0, (N, nc, 1)) * mdir
    d = oracle.OracleData.build(model, base_position=pos, base_quaternion=quat, joint_positions=s, base_linear_velocity=vel,
                                tangential_deformation=m, velocity_representation=VelRepr.Inertial, dtype=dtype)  # fmt: skip
    # (no angular velocity: the stored inertial-fixed velocity is the same three numbers in every representation's frame
    # of reference; only the label changes what the device converts on the way in and out)
    return dataclasses.replace(d, velocity_representation=rep), sink, vs


# ---- the case table ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    row: str                 # row of the table (A .. G)
    name: str                # model: box, anymal, icub, icub80, fixedcart
    terrain: str             # flat, plane, hf
    dtype: type
    pq: tuple | None = None  # contact exponents (None: the model's defaults, p = q = 0.5)
    mu0: bool = False
    rk4: bool = False
    rep: str = VelRepr.Inertial

    @property
    def N(self) -> int:
        return N_BY_MODEL.get(self.name, N_ENV)

    @property
    def key(self) -> str:
        parts = [self.row, self.name, self.terrain, np.dtype(self.dtype).name]
        parts += [f"p{self.pq[0]}q{self.pq[1]}"] if self.pq else []
        parts += ["mu0"] if self.mu0 else []
        parts += ["rk4"] if self.rk4 else []
        parts += [self.rep] if self.rep != VelRepr.Inertial else []
        return "-".join(parts)

    @property
    def family(self) -> str:
        return self.name


BOTH, F64 = (np.float64, np.float32), (np.float64,)
TERRAINS = ("flat", "plane", "hf")
CASES = [Case("A", n, t, dt) for n in ("box", "anymal", "icub") for t in TERRAINS for dt in BOTH]
CASES += [Case("B", n, t, dt, pq=(0.7, 0.3)) for n in ("box", "icub") for t in TERRAINS for dt in BOTH]
CASES += [Case("C", "box", "plane", np.float64, pq=pq) for pq in ((0.5, 0.25), (1.0, 1.0))]
CASES += [Case("D", n, t, dt, mu0=True) for n in ("box", "anymal") for t in ("flat", "plane") for dt in BOTH]
CASES += [Case("E", "icub80", "plane", np.float64, pq=pq, rk4=rk4) for rk4 in (False, True) for pq in (None, (0.7, 0.3))]
CASES += [Case("F", n, "plane", np.float64, pq=pq, rk4=True) for n in ("box", "icub") for pq in (None, (0.7, 0.3))]
CASES += [Case("G", "fixedcart", t, dt) for t in ("flat", "plane") for dt in BOTH]
# cases A and B of the box and the humanoid on the plane, in the two other velocity representations (device only: the
# emulation's harness evaluates the inertial representation)
REP_CASES = [dataclasses.replace(c, rep=rep) for c in CASES if c.row in "AB" and c.terrain == "plane" and c.name in ("box", "icub")
             for rep in (VelRepr.Body, VelRepr.Mixed)]  # fmt: skip
BY_KEY = {c.key: c for c in CASES + REP_CASES}
assert len(BY_KEY) == len(CASES) + len(REP_CASES)
EULER_KEYS = [c.key for c in CASES if not c.rk4]
RK4_KEYS = [c.key for c in CASES if c.rk4]
REP_KEYS = [c.key for c in REP_CASES]


def base_model(zoo, name):
    if name == "icub80":
        if "icub80" not in zoo._cache:
            zoo._cache["icub80"] = ja.JaxSimModel.build_from_model_description(robots.icub23_urdf(sole_boxes_per_foot=5))
        return zoo._cache["icub80"]
    if name == "fixedcart":
        # the cartpole with collision shapes and SoftContacts on all eight corners of the cart: a fixed-base mechanism
        # whose collidable points reach the ground (the URDF behind helpers.fixed_cart_model)
        if "fixedcart" not in zoo._cache:
            zoo._cache["fixedcart"] = ja.JaxSimModel.build_from_model_description(robots.cartpole_urdf(with_collisions=True))
        assert not zoo._cache["fixedcart"].floating_base()
        return zoo._cache["fixedcart"]
    return zoo(name)


def case_models(zoo, case: Case):
    """(model on the product's terrain, the same model on the oracle's statement of it)."""
    base = base_model(zoo, case.name)
    cp = base.contact_params
    kw = dict(K=cp.K, D=cp.D, mu=cp.mu, p=cp.p, q=cp.q)
    if case.rk4:
        kw.update(RK4_SOFT)
    if case.pq:
        kw.update(p=case.pq[0], q=case.pq[1])
    if case.mu0:
        kw.update(mu=0.0)
    changes = dict(contact_params=ja.SoftContactsParams.build(**kw))
    if case.rk4:
        changes["integrator"] = ja.IntegratorType.RungeKutta4
    base = helpers.with_params(base, **changes)
    if case.terrain == "flat":
        return base, base
    if case.terrain == "plane":
        m = helpers.with_params(base, terrain=ja.PlaneTerrain.build(PLANE["height"], normal=PLANE["normal"]))
        return m, m
    t, g = hfc.edge_field()
    return helpers.with_params(base, terrain=t), helpers.with_params(base, terrain=g)


_CASE_CACHE: dict = {}


def case_data(zoo, key: str) -> dict:
    """Everything a case needs, computed once per process and left unchanged: the two models, the state, the per-environment
    scales, the classifier's view of the state (input conditions asserted) and the fp64 truth."""
    if key in _CASE_CACHE:
        return _CASE_CACHE[key]
    case = BY_KEY[key]
    model, model_ref = case_models(zoo, case)
    d, sink, vs = regime_states(model_ref, case.N, SEED, SINK_LO[np.dtype(case.dtype)], case.dtype, case.rep, MU0_SCALE if case.mu0 else None)
    d64 = helpers.upcast(d, model_ref)
    R = regimes(model_ref, d64)
    require(case, model, R)
    out = dict(case=case, model=model, model_ref=model_ref, d=d, d64=d64, sink=sink, vs=vs, R=R, truth=truth_of(model_ref, d64),
               f_scale=model.contact_params.K * sink**1.5)  # fmt: skip
    _CASE_CACHE[key] = out
    return out


# ---- the input conditions ------------------------------------------------------------------------------------------------
def require(case: Case, model, R: dict) -> None:
    """A case that loses a condition fails here, before anything is compared."""
    c = counts(R)
    ctx = (case.key, c)
    if case.name == "icub80":
        lay = st.StateLayout.of(model)
        assert lay.n_points == 80, lay
        en = np.flatnonzero(np.asarray(model.kin_dyn_parameters.contact_enabled, dtype=bool))
        behind = en >= 32  # points of the chunks behind the first lane group
        for k in ("stick", "slip", "liftoff"):
            assert int(R[k][:, behind].sum()) >= 2, (k, ctx)
    if case.mu0:
        loaded = R["contact"] & (R["ft"] > 0)
        assert (R["slipping"] == loaded).all() and int(loaded.sum()) >= 10, ctx
        need = ("liftoff", "rest")
    elif case.name == "fixedcart":
        need = ("stick", "slip")  # row G asks for these two (measured: every regime is reached all the same)
    else:
        need = ("stick", "slip", "liftoff", "rest")
    for k in need:
        assert c[k] >= 5, (k, ctx)
    assert int((R["airborne"] & (R["m_norm"] > 0)).sum()) >= 5, ctx
    if np.dtype(case.dtype) == np.float64:
        assert int((R["contact"] & (R["delta"] < 1e-4)).sum()) >= 5, ctx
    else:
        assert int((np.abs(R["h"]) < 1e-6).sum()) == 0, ctx  # no grazing point: float32 cannot tell which side it is on
    assert int((R["delta"] > 1e-3).sum()) >= 3, ctx
    if case.terrain != "flat" and not case.mu0:
        tilted = np.abs(R["m_n"]) > 0.1 * R["m_norm"]
        assert int((R["stick"] & tilted).sum()) >= 5 and int((R["slip"] & tilted).sum()) >= 5, ctx


# ---- truth, metrics, gates -----------------------------------------------------------------------------------------------
def derivative_block(model, xd: dict) -> np.ndarray:
    keys = ("base_position", "base_quaternion", "joint_positions", "base_linear_velocity", "base_angular_velocity", "joint_velocities", "tangential_deformation")
    return st.pack_state(st.StateLayout.of(model), dtype=np.asarray(xd["base_position"]).dtype, **{k: xd[k] for k in keys})


def truth_of(model_ref, d) -> dict:
    """The oracle's answers for a state, in the precision of the state: the derivative block of system_dynamics (inertial
    representation, as the product evaluates it), the link wrenches and m_dot of link_contact_forces, one step."""
    d_in = dataclasses.replace(d, velocity_representation=VelRepr.Inertial)
    W, md = oracle.refstep.link_contact_forces(model_ref, d_in)
    return dict(block=derivative_block(model_ref, oracle.refstep.system_dynamics(model_ref, d_in)), W=W, m_dot=md,
                step=helpers.odata_to_block(model_ref, oracle.step(model_ref, d)))  # fmt: skip


def own_scale(a, ref, scale) -> float:
    """Per environment max |a - ref| / max(max |ref|, s_e), worst environment: the error of a per-point quantity on the
    environment's natural scale s_e -- the sliding speed vs_e = (K / D) sink_e for m_dot, the contact force
    K sink_e^1.5 for wrenches -- never on the scale of an acceleration of the same block."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return float(np.max(np.abs(a - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), scale)))


def m_rows(model, block):
    """[N, n_points, 3] out of the rows of m of a [rows, N] block."""
    lay = st.StateLayout.of(model)
    return np.asarray(block)[lay.row_m :].T.reshape(block.shape[1], lay.n_points, 3)


QUANTITIES = ("block", "m_dot", "wrench", "wrench_own", "step", "step_m")


def errors(cd: dict, *, block=None, m_dot=None, W=None, step=None, truth=None) -> dict:
    """Errors of whichever answers are given against the fp64 truth of the case, quantity by quantity: ``block``, ``wrench``,
    ``step``: helpers.rel_err; ``m_dot``, ``wrench_own``: own_scale; ``step_m``: the rows of m of the stepped state as a
    rate, (m+ - m+_ref) / dt, on the scale of vs_e."""
    t = truth or cd["truth"]
    model, out = cd["model"], {}
    if block is not None:
        out["block"] = helpers.rel_err(block, t["block"])
    if m_dot is not None:
        out["m_dot"] = own_scale(m_dot, t["m_dot"], cd["vs"])
    if W is not None:
        out["wrench"] = helpers.rel_err(W, t["W"])
        out["wrench_own"] = own_scale(W, t["W"], cd["f_scale"])
    if step is not None:
        out["step"] = helpers.rel_err(step, t["step"])
        out["step_m"] = own_scale(m_rows(model, step) / model.time_step, m_rows(model, t["step"]) / model.time_step, cd["vs"])
    return out


_F32_CACHE: dict = {}


def fp32_reference_errors(zoo, family: str) -> dict:
    """Per quantity, the worst error over the family's float32 cases of the REFERENCE formulation evaluated in float32 (the
    oracle on the float32 state, not upcast) against the fp64 truth, in the metric of ``errors``; and per case under
    ``cases``.  Never the kernel's error: the float32 gates are three times these figures (the project's rule: measured
    worst x 3)."""
    if family in _F32_CACHE:
        return _F32_CACHE[family]
    worst, per_case = {q: 0.0 for q in QUANTITIES}, {}
    for c in CASES:
        if c.family != family or np.dtype(c.dtype) != np.float32:
            continue
        cd = case_data(zoo, c.key)
        t32 = truth_of(cd["model_ref"], cd["d"])
        assert t32["block"].dtype == np.float32 and t32["step"].dtype == np.float32
        e = errors(cd, block=t32["block"], m_dot=t32["m_dot"], W=t32["W"], step=t32["step"])
        # the states pin something: on its own scale the float32 reference is within 1e-2 of the truth
        assert e["m_dot"] < 1e-2 and e["wrench_own"] < 1e-2, (c.key, e)
        per_case[c.key] = e
        for q in QUANTITIES:
            worst[q] = max(worst[q], e[q])
    out = dict(worst, cases=per_case)
    _F32_CACHE[family] = out
    return out


def gate(zoo, case: Case, quantity: str) -> float:
    if np.dtype(case.dtype) == np.float64:
        return helpers.FP64_TOL
    return 3.0 * fp32_reference_errors(zoo, case.family)[quantity]


def measured(key: str, value: float, gate_: float | None) -> float:
    """Print a figure next to its gate before it is asserted (and log it: helpers.note); returns the figure."""
    print(f"[soft regimes] {key}: {value:.3e} (gate {'none' if gate_ is None else format(gate_, '.1e')})")
    helpers.note(key, value)
    return value


GATED = ("block", "m_dot", "wrench", "step", "step_m")  # (wrench_own in fp64: printed and logged, not gated)


def check(zoo, cd: dict, who: str, **answers) -> dict:
    """Measure every quantity of ``answers``, print it with its gate, then assert the gated ones."""
    case = cd["case"]
    e = errors(cd, **answers)
    f64 = np.dtype(case.dtype) == np.float64
    gates = {q: (None if (q == "wrench_own" and f64) else gate(zoo, case, q)) for q in e}
    for q, v in e.items():
        measured(f"{who} {q} {case.key}", v, gates[q])
    for q, v in e.items():
        if gates[q] is not None:
            assert v < gates[q], (who, q, case.key, v, gates[q])
    return e


def rest_environments(cd: dict) -> np.ndarray:
    return np.flatnonzero(np.arange(cd["case"].N) % 5 == 3)


def assert_rest(cd, m_dot):
    """v = 0 and m = 0: the rate of every point of a rest environment is zero exactly, in both precisions."""
    rest = rest_environments(cd)
    assert (np.asarray(m_dot)[rest] == 0).all(), np.abs(np.asarray(m_dot)[rest]).max()


# ---- row H: a point exactly on the ground, and one ulp either side -----------------------------------------------------------
def grazing_case(zoo, dtype):
    """(box model, state of 4 environments, expected m_dot [4, 8, 3], in-contact flag per environment): an axis-aligned box
    whose base height is its half height exactly, one ulp above, one ulp below and 1 mm below, with m != 0 on every
    corner and a small base velocity (downwards, so that the point one ulp inside has a normal force and sticks).
    The float32 box is 0.25 x 0.125 x 0.125: its half height is a float32 number, so kernel and oracle see the same zero."""
    dtype = np.dtype(dtype)
    key = f"graze-{dtype.name}"
    if key not in zoo._cache:
        size = (0.3, 0.2, 0.1) if dtype == np.float64 else (0.25, 0.125, 0.125)
        zoo._cache[key] = ja.JaxSimModel.build_from_model_description(robots.box_urdf(size=size))
    model = zoo._cache[key]
    half = dtype.type(-np.asarray(model.kin_dyn_parameters.contact_point)[:, 2].min())
    assert float(half) == -np.asarray(model.kin_dyn_parameters.contact_point)[:, 2].min()  # representable
    z = np.array([half, np.nextafter(half, dtype.type(1)), np.nextafter(half, dtype.type(0)), half - dtype.type(1e-3)], dtype=dtype)
    N = 4
    pos = np.zeros((N, 3), dtype=dtype)
    pos[:, 2] = z
    rng = np.random.default_rng(17)
    vel = np.tile(np.array([1.0e-3, -0.5e-3, -1.0e-2]), (N, 1))
    m = 2e-6 * rng.uniform(0.5, 1.0, (N, 8, 1)) * np.stack([np.cos(a := rng.uniform(0, 6.28, (N, 8))), np.sin(a), 0.3 * rng.uniform(-1, 1, (N, 8))], -1)
    d = oracle.OracleData.build(model, base_position=pos, base_linear_velocity=vel, tangential_deformation=m,
                                velocity_representation=VelRepr.Inertial, dtype=dtype.type)  # fmt: skip
    d64 = helpers.upcast(d, model)
    R = regimes(model, d64)
    low = np.asarray(model.kin_dyn_parameters.contact_point)[:, 2] < 0
    # on the ground exactly | one ulp above | one ulp inside (the differences of neighbouring numbers are exact)
    assert (R["h"][0, low] == 0).all() and (R["h"][1, low] == float(half) - float(z[1])).all() and (R["h"][2, low] == float(half) - float(z[2])).all()
    assert float(z[1]) > float(half) > float(z[2]) and float(half) - float(z[2]) <= float(np.spacing(half))
    assert (R["h"][:, ~low] < 0).all() and (R["m_norm"] > 0).all()
    assert R["stick"][2:, low].all() and not R["contact"][:2].any()
    cp = model.contact_params
    m64 = d64.tangential_deformation
    expected = -(cp.K / cp.D) * m64  # no contact: the spring relaxes
    for e in (2, 3):  # sticking on flat ground: (v_x, v_y, -(K / D) m_z)
        expected[e][low, :2] = d64.base_linear_velocity[e, :2]
    return model, d, expected, np.array([False, False, True, True])


def check_grazing(model, d, expected, touching, m_dot, W, dtype):
    m_dot, W = np.asarray(m_dot, np.float64), np.asarray(W, np.float64)
    assert (W[~touching] == 0).all() and (np.abs(W[touching, 0, 2]) > 0).all()
    # the two closed forms, to a few roundings of the precision (K / D and one product)
    rtol = 8 * np.finfo(dtype).eps
    np.testing.assert_allclose(m_dot, expected, rtol=rtol, atol=0)
    ref_W, ref_md = oracle.refstep.link_contact_forces(model, helpers.upcast(d, model))
    tol = helpers.tol_of(dtype, "box")
    assert helpers.rel_err(m_dot, ref_md) < tol
    # (one float32 ulp of depth, 4e-9 m, is less than the float32 eps inside sqrt(delta + eps), which the law takes from
    # the precision it runs in: that environment's force has the float32 reference as its truth)
    every = np.dtype(dtype) == np.float64
    assert helpers.rel_err(W[[0, 1, 3]] if not every else W, ref_W[[0, 1, 3]] if not every else ref_W) < tol
    if not every:
        assert helpers.rel_err(W[2], oracle.refstep.link_contact_forces(model, d)[0][2]) < tol
