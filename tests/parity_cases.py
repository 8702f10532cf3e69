"""TEST INFRASTRUCTURE: the one statement of the parity cases of tests/test_emulation_parity.py (host emulation) and
tests/test_gpu_parity.py (device) -- model lists, contact cases, case builders, the golden-vector helpers and the truth of
the system_dynamics comparisons.  Plain data and builders: nothing here needs the emulation harness or a device, so the
build step, the tools and every other test module read the cases from here.  N, seeds, dtypes, enabled points and contact
parameters are arguments: each side passes its own.
"""

from __future__ import annotations

import pathlib

import numpy as np
import pytest

import helpers
import jaxsim_amd as ja
import maxcoord
import oracle
from jaxsim_amd import robots
from oracle import VelRepr

REPS = [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed]
REPR_CODE = {VelRepr.Inertial: 0, VelRepr.Body: 1, VelRepr.Mixed: 2}
ALL = ["box", "sphere", "pendulum", "double_pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub", "icub16"]
RK4_MODELS = ["box", "sphere", "pendulum", "cartpole", "chain9f", "anymal", "icub16"]  # sphere: 50 points -> 64 lanes
ROW_MODELS = ["double_pendulum", "cartpole", "chain5", "anymal", "icub", "icub16"]

# ---- Runge-Kutta 4 (reference: api/integrators.py:91-167) -----------
# Explicit RK4 leaves its stability region on the zoo's default contact stiffness (K = 1e6,
# D = 2000 at dt = 1 ms amplify light links by 1e7 per step, in the reference too), which
# would turn a parity check into a chaos check: every Runge-Kutta case of the suite uses a softer ground.
RK4_SOFT = dict(K=2e4, D=60.0, mu=0.6)


def rk4(model):
    return helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4, contact_params=ja.SoftContactsParams.build(**RK4_SOFT))


def icub80():
    return ja.JaxSimModel.build_from_model_description(robots.icub23_urdf(sole_boxes_per_foot=5))  # 80 points on two links


def icub80_data(model, N, dtype=np.float64):
    return oracle.random_model_data(model, batch_size=N, seed=3, dtype=dtype, base_pos_bounds=((-1, -1, 0.56), (1, 1, 0.66)),
                                    base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3)))  # fmt: skip


def quadruped_200():
    """The quadruped with a 50-point sphere at every shank tip: 200 collidable points, like the real robot's URDF
    (parsers/rod/utils.py:200-204 turns a sphere collision shape into 50 Fibonacci points)."""
    return ja.JaxSimModel.build_from_model_description(robots.anymal12_urdf(foot_shape="sphere"))


def sine_field(extent=4.0, spacing=0.05, amp=0.04):
    """A rolling terrain: z = amp (sin(2.1 x + 0.3) cos(1.7 y) + 0.3 sin(3.3 y)), sampled on a 5 cm grid over [-extent, extent]^2
    (slopes up to ~10 degrees: the normal is far from +z).  Returns (product terrain, oracle terrain of the SAME grid, function)."""
    from oracle import refterrain

    fn = lambda x, y: amp * (np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.3 * np.sin(3.3 * y))  # noqa: E731
    t = ja.HeightFieldTerrain.from_function(fn, x_range=(-extent, extent), y_range=(-extent, extent), spacing=spacing)
    return t, refterrain.GridTerrain(np.array(t._heights), t._origin, t._spacing, t.delta), fn


# ---- RigidContacts (reference: rbda/contacts/rigid.py:176-539; BASELINE.json config 5) ----
# The kernel solves the reduced statement of the reference's QP (oracle/refrigid.py REDUCED_QP);
# against that statement the interior-point iterates are the same up to rounding, so the fp64
# check is tight.  tests/test_oracle_rigid.py bounds the distance between the two statements.
RIGID_CASES = {
    "box4": ("box", [0, 1, 2, 3], dict(K=1e5)),
    "anymal16": ("anymal", helpers.ANYMAL_FEET_16, dict(K=1e4, D=1e2)),
    "anymal4": ("anymal", helpers.ANYMAL_FEET_4, dict()),
    "chain9f6": ("chain9f", [0, 1, 2, 3, 8, 9], dict(K=1e3, mu=0.8)),
    "serial12f": ("serial12f", list(range(16)), dict(K=1e3, mu=0.8)),  # two contact links eleven joints apart
    "icub8": ("icub16", [0, 1, 2, 3, 8, 9, 10, 11], dict(K=1e4)),
    "planar_biped": ("planar_biped", list(range(16)), dict(K=1e4)),  # [round 5] six parallel joint axes between the two feet
    "planar10f": ("planar10f", list(range(16)), dict(K=1e3, mu=0.8)),
    # <= 4 points in a 32-lane group: the row-distributed register solver with the general Delassus sweeps
    # (two points per foot: no merged sweep)
    "icub4": ("icub16", [2, 9, 10, 11], dict(K=1e4)),
    "anymal2": ("anymal", [0, 16], dict()),  # merged sweeps and the 12-row solver with identity padding
}

# ---- RelaxedRigidContacts (reference: rbda/contacts/relaxed_rigid.py; the model of the
# reference's own test_simulation_step benchmark, tests/test_benchmark.py:142-152) ----
RELAXED_CASES = {
    "box4": ("box", [0, 1, 2, 3], dict()),
    "box8": ("box", list(range(8)), dict(mu=0.5)),
    "anymal16": ("anymal", helpers.ANYMAL_FEET_16, dict(mu=0.5)),
    "anymal4": ("anymal", helpers.ANYMAL_FEET_4, dict(time_constant=0.01, damping_coefficient=0.7, power=1.5)),
    "chain9f6": ("chain9f", [0, 1, 2, 3, 8, 9], dict(mu=0.8, d_min=0.5, d_max=0.99, width=5e-3, midpoint=0.3)),
    "serial12f": ("serial12f", list(range(16)), dict(mu=0.8, d_min=0.5, d_max=0.99, width=5e-3, midpoint=0.3)),
    "icub16": ("icub16", list(range(16)), dict(mu=0.5)),
    # [r4] the reference's DEFAULT parameters (mu = 0.005: the regulariser is five orders below the Delassus entries) on two
    # links: solved in the tree in fp64 (jxs_pack.h)
    "icub16d": ("icub16", list(range(16)), dict()),
    # [round 5] parallel joint axes between the contact links
    "planar_biped": ("planar_biped", list(range(16)), dict(mu=0.5)),
    "planar10f": ("planar10f", list(range(16)), dict(mu=0.8, d_min=0.5, d_max=0.99, width=5e-3, midpoint=0.3)),
}

# ---- [round 6] links with more than six children (VERDICT r5 missing 3: kMaxChildren 6 -> 12) ----
OCTOPOD_FEET_4 = [0, 8, 16, 24]                                           # one bottom corner per foot
OCTOPOD_FEET_16 = [8 * f + c for f in range(4) for c in range(4)]          # the four bottom corners of every foot


@pytest.fixture()
def reduced_qp():
    """The kernel solves the reduced statement of the reference's QP (oracle/refrigid.py)."""
    from oracle import refrigid

    refrigid.REDUCED_QP = True
    yield refrigid
    refrigid.REDUCED_QP = False


def contact_model(kind, base, idx, **params):
    """``base`` with RigidContacts (kind "rigid") or RelaxedRigidContacts ("relaxed") on the enabled points ``idx``."""
    return (helpers.rigid_model if kind == "rigid" else helpers.relaxed_model)(base, idx, **params)


def rigid_case(models, key, N, seed, dtype=np.float64, build=None, **data_kw):
    """(model, random states) of RIGID_CASES[key]; ``build`` goes to RigidContacts.build (solver options), ``data_kw`` to
    the zoo's random_data (rep=...)."""
    name, idx, params = RIGID_CASES[key]
    return helpers.rigid_model(models(name), idx, build=build, **params), models.random_data(name, N, seed=seed, dtype=dtype, **data_kw)


def relaxed_case(models, key, N, seed, dtype=np.float64, **data_kw):
    """(model, random states) of RELAXED_CASES[key]."""
    name, idx, params = RELAXED_CASES[key]
    return helpers.relaxed_model(models(name), idx, **params), models.random_data(name, N, seed=seed, dtype=dtype, **data_kw)


def contact_case(models, kind, key, N, seed, dtype=np.float64, **data_kw):
    return (rigid_case if kind == "rigid" else relaxed_case)(models, key, N, seed, dtype, **data_kw)


def rollout_case(models, name, kind, N, seed):
    """(model, states) of the controlled / recorded rollout tests: a zoo model or the 80-point humanoid ("icub80") as is
    ("euler"), on the Runge-Kutta ground ("rk4"), with RigidContacts on one corner per foot of the quadruped ("rigid"), or
    with half of its points disabled ("disabled")."""
    if name == "icub80":
        model = icub80()
        d = icub80_data(model, N)
    else:
        model = models(name)
        d = models.random_data(name, N, seed=seed)
    if kind == "rk4":
        model = rk4(model)
    if kind == "rigid":
        model = helpers.rigid_model(model, helpers.ANYMAL_FEET_4, K=1e4, D=2e2)
    if kind == "disabled":
        model = helpers.enable_points(model, [0, 1, 2, 3, 8, 9, 10, 11])
    return model, d


def standing_case(models, kind, name, idx, N, dtype):
    """Standing states with every bottom point of every foot in contact (test_standing_on_every_sole_point*)."""
    model = contact_model(kind, models(name), idx, **(dict(mu=0.5) if kind == "relaxed" else dict(K=1e4, D=1e2)))
    return model, helpers.standing_data(model, N, seed=5, dtype=dtype, noise=0.003)


def settling_box(models, kind, integrator=None):
    """The box of the reference's settling tests (tests/test_simulations.py:245-346) at the solver tolerance they use."""
    build = dict(solver_options={"solver_tol" if kind == "rigid" else "tol": 1e-3})
    model = contact_model(kind, models("box"), [0, 1, 2, 3], build=build, **(dict(K=1e5) if kind == "rigid" else {}))
    return model if integrator is None else helpers.with_params(model, integrator=integrator)


def tumbling_box(models, kind):
    """(model, state) of a box dropped on an edge with forward speed."""
    model = contact_model(kind, models("box"), [0, 1, 2, 3], **(dict(K=1e5) if kind == "rigid" else dict(mu=0.5)))
    q = oracle.refmath.quaternion_from_euler_xyz(np.array([[0.3, 0.2, 0.1]]))
    return model, oracle.OracleData.build(model, base_position=[0, 0, 0.3], base_quaternion=q, base_linear_velocity=[0.5, 0, 0])


def fixed_cart_case(kind, N, base_velocity, dtype=np.float64):
    """A FIXED-base model (a cart on a rail touching the ground) with RigidContacts / RelaxedRigidContacts."""
    model = helpers.fixed_cart_model(kind) if kind == "rigid" else helpers.fixed_cart_model(kind, mu=0.5)
    return model, helpers.fixed_cart_data(model, N, seed=3, dtype=dtype, base_velocity=base_velocity)


def sphere50_model(models, kind):
    """The reference's 50-point sphere collision shape (parsers/rod/utils.py:200-204) with every point enabled."""
    return contact_model(kind, models("sphere"), list(range(50)), **(dict(K=1e5) if kind == "rigid" else dict(mu=0.5)))


def sphere50_data(model, N, dtype=np.float64):
    return oracle.random_model_data(model, batch_size=N, seed=6, dtype=dtype, base_pos_bounds=((-1, -1, 0.04), (1, 1, 0.07)),
                                    base_rpy_bounds=((-3, -3, -3), (3, 3, 3)))  # sunk 3 .. 6 cm: the bottom cap of points touches


def octopod_case(models, kind, idx, N, dtype=np.float64):
    model = contact_model(kind, models("octopod"), idx, **(dict(K=1e4, D=1e2) if kind == "rigid" else dict(mu=0.5)))
    return model, models.random_data("octopod", N, seed=5, dtype=dtype)


# ---- committed golden vectors (tests/golden/*.npz, generated by the oracle) ---------------------------------------------
GOLD = pathlib.Path(__file__).resolve().parent / "golden"
INTEGRATOR_GOLDEN = {
    "relaxed_rk4_anymal": ("relaxed", "anymal"),
    "relaxed_rk4fast_anymal": ("relaxed", "anymal"),
    "rigid_rk4_box": ("rigid", "box"),
    "rigid_rk4fast_box": ("rigid", "box"),
}


def load(name):
    return dict(np.load(GOLD / f"{name}.npz"))


def rk4_golden_model(models, name):
    return rk4(models(name))


def rigid_golden_model(models, name, g):
    return helpers.rigid_model(models(name), [int(i) for i in g["enabled"]], K=float(g["K"]), D=float(g["D"]))


def relaxed_golden_model(models, name, g):
    return helpers.relaxed_model(models(name), [int(i) for i in g["enabled"]], mu=float(g["mu"]))


def integrator_golden_model(models, tag, g):
    kind, name = INTEGRATOR_GOLDEN[tag]
    idx = [int(i) for i in g["enabled"]]
    base = helpers.relaxed_model(models(name), idx, mu=0.4) if kind == "relaxed" else helpers.rigid_model(models(name), idx, K=1e5)
    return helpers.with_params(base, integrator=ja.IntegratorType(int(g["integrator"])))


# ---- [round 6] system_dynamics / link_contact_forces (SURVEY section 8(a) rows E and I as callable entries) -----------
# reference: src/jaxsim/api/ode.py:16-225, src/jaxsim/api/contact.py:514-603; the kernel modes MODE_DYN / MODE_DYN_RIGID
def link_contact_forces(model, d, tau, f):
    """Link contact wrenches [N, nL, 6] of the oracle, whatever the contact model (zero without collidable points)."""
    if oracle.refstep.is_rigid_contact_model(model):
        from oracle import refrigid

        return refrigid.link_contact_forces(model, d, link_forces=f, joint_torques=tau)[0]
    if oracle.refstep.is_relaxed_rigid_contact_model(model):
        from oracle import refrelaxed

        return refrelaxed.link_contact_forces(model, d, link_forces=f, joint_torques=tau)[0]
    if model.kin_dyn_parameters.number_of_collidable_points() == 0:
        return np.zeros((d.batch_size, model.number_of_links(), 6))
    return oracle.refstep.link_contact_forces(model, d)[0]


def dyn_reference(model, d, tau, f):
    """(derivative block [rows, N], link contact wrenches [N, nL, 6]) of the oracle for inertial data."""
    xd = oracle.refstep.system_dynamics(model, d, link_forces=f, joint_torques=tau)
    blk = helpers.st.pack_state(
        helpers.st.StateLayout.of(model), base_position=xd["base_position"], base_quaternion=xd["base_quaternion"],
        joint_positions=xd["joint_positions"], base_linear_velocity=xd["base_linear_velocity"],
        base_angular_velocity=xd["base_angular_velocity"], joint_velocities=xd["joint_velocities"],
        tangential_deformation=xd["tangential_deformation"], dtype=np.float64,
    )  # fmt: skip
    return blk, link_contact_forces(model, d, tau, f)


def dyn_err(a, ref, dtype, env_axis=0):
    """Metric of the derivative / wrench comparisons; ``env_axis`` is the environment axis of the two arrays (0 for the
    API's [N, ...] arrays, -1 for the [rows, N] blocks of the emulation).  fp64: helpers.rel_err, element by element.
    fp32: the worst element error of an environment relative to the LARGEST entry of that environment's reference
    (at least 1).  A 1e6 N/m^1.5 contact turns the 6e-8 m an fp32 foot height is known to into a force error of 1e-3 of
    the contact force, which reaches every acceleration of the tree -- the small ones included; the step's gates see the
    same error times dt = 1e-3 against states of order one, i.e. the same scale."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if np.dtype(dtype) == np.float64:
        return helpers.rel_err(a, ref)
    a, ref = np.moveaxis(a, env_axis, 0), np.moveaxis(ref, env_axis, 0)
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return float(np.max(np.abs(a - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1)))) if a.size else 0.0


# ---- the models and the truth of the maximal-coordinate checks (tests/maxcoord.py itself imports nothing of the project) ----
MAXCOORD_TEXTS = {
    "cartpole": lambda: robots.cartpole_urdf(),
    "pendulum": lambda: robots.single_pendulum_urdf(),
    "double_pendulum": lambda: robots.double_pendulum_urdf(),
    "chain5": lambda: robots.chain_urdf(5, fixed_base=True, seed=1),
    "chain9f": lambda: robots.chain_urdf(9, fixed_base=False, seed=2),
    "box": lambda: robots.box_urdf(),
    "anymal": lambda: robots.anymal12_urdf(),
    "icub": lambda: robots.icub23_urdf(),
    "octopod": lambda: robots.hub_urdf(8, 2, foot_boxes=4, seed=1),
    "lumped7f": lambda: robots.lumped_tree_urdf(7, seed=0),
    "lumped12f": lambda: robots.lumped_tree_urdf(12, seed=2),
    "lumped5": lambda: robots.lumped_tree_urdf(5, seed=1, fixed_base=True),
}
OFFSET_BASE = ("pendulum", "chain5", "double_pendulum")  # fixed bases placed off the world origin: no link wrenches (quirk 12)
_MAXCOORD_MODELS = {}


def maxcoord_case(name, N, seed, dtype=np.float64):
    if name not in _MAXCOORD_MODELS:
        text = MAXCOORD_TEXTS[name]()
        _MAXCOORD_MODELS[name] = (text, ja.JaxSimModel.build_from_model_description(text))
    text, model = _MAXCOORD_MODELS[name]
    d = oracle.random_model_data(model, batch_size=N, seed=seed, dtype=dtype, velocity_representation=VelRepr.Mixed)
    if not model.floating_base():  # ABA keeps the base of a fixed-base model at rest (rbda/aba.py:109-121)
        d.base_linear_velocity[:] = 0
        d.base_angular_velocity[:] = 0
    rng = np.random.default_rng(seed + 1)
    tau = rng.uniform(-3, 3, size=(N, model.dofs())).astype(dtype)
    f = rng.uniform(-5, 5, size=(N, model.number_of_links(), 6)).astype(dtype)
    if name in OFFSET_BASE:
        f[:] = 0
    return text, model, d, tau, f


def maxcoord_truth(text, model, d, tau, f):
    """(base acceleration in MIXED representation [N, 6], joint accelerations [N, n] in the model's joint order) from
    tests/maxcoord.py; the inputs are read in float64 whatever the dtype of the state."""
    jn, lnm = model.joint_names(), model.link_names()
    N = d.base_position.shape[0]
    vd, sdd = np.zeros((N, 6)), np.zeros((N, len(jn)))
    bv = d.base_velocity(VelRepr.Mixed).astype(np.float64)  # (the data object STORES the inertial-fixed velocity, api/data.py:151-156)
    for e in range(N):
        ba, acc = maxcoord.forward_dynamics(
            text, base_position=d.base_position[e].astype(np.float64), base_quaternion=d.base_quaternion[e].astype(np.float64),
            base_linear_velocity=bv[e, :3], base_angular_velocity=bv[e, 3:],
            joint_positions=dict(zip(jn, d.joint_positions[e].astype(np.float64))), joint_velocities=dict(zip(jn, d.joint_velocities[e].astype(np.float64))),
            joint_forces=dict(zip(jn, tau[e].astype(np.float64))),
            link_wrenches={n: (f[e, i, :3].astype(np.float64), f[e, i, 3:].astype(np.float64)) for i, n in enumerate(lnm)}, gravity=model.gravity)  # fmt: skip
        vd[e] = ba
        sdd[e] = [acc[n] for n in jn]
    return vd, sdd
