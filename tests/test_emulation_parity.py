"""CPU parity: the kernel core (jaxsim_amd/csrc/jxs_core.h), compiled against the host
lockstep lane backend, versus the oracle.  Same tables, same shuffles, same level loops as
the gfx950 kernels -- only the lane backend differs -- so this is the -m "not gpu" check of
the kernel *logic*.  Tolerances (helpers.py): fp64 1e-10, fp32 1e-3 worst-case (2e-2 for the noise-limited chain9f) relative to the fp64 oracle on the same inputs.
"""

import dataclasses
import numpy as np
import pytest

import emul_binding as eb
import helpers
import oracle
import parity_cases as pc
from oracle import VelRepr
from parity_cases import ALL, OCTOPOD_FEET_4, OCTOPOD_FEET_16, RELAXED_CASES, REPR_CODE, RIGID_CASES, RK4_MODELS, ROW_MODELS, reduced_qp  # noqa: F401


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_step_matches_oracle(models, name, dtype):
    model = models(name)
    N = 6
    d = models.random_data(name, N, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T,
                 link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[d.velocity_representation])  # fmt: skip
    assert out.dtype == dtype
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)


def test_fp32_not_worse_than_reference_formulation(models):
    """fp32: distance to the fp64 truth of (a) the kernel core (anchored ABA) and (b) the reference's own
    body-frame formulation evaluated in fp32 (the oracle run with float32 arrays): the worst environment
    within the stated tolerance, the 90th percentile within a small factor of the reference formulation's, the
    MEDIAN environment of the humanoid below 1e-6 (round 1, one reference point for the whole tree: 9e-6)."""
    for name in ("anymal", "icub", "chain9f"):
        model = models(name)
        N = 64
        d = models.random_data(name, N, seed=4, dtype=np.float32)
        truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d)))
        per_env = lambda blk: np.max(np.abs(blk.astype(np.float64) - truth) / np.maximum(1.0, np.abs(truth)), axis=0)  # noqa: E731
        ours = per_env(eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d)))
        theirs = per_env(helpers.odata_to_block(model, oracle.step(model, d)))
        assert ours.max() < helpers.tol_of(np.float32, name)
        # the worst environment is decided by how many digits of a millimetre penetration survive (both
        # formulations lose them alike): compare the bulk of the distribution
        assert np.percentile(ours, 90) <= 3.0 * np.percentile(theirs, 90) + 1e-6, (name, np.percentile(ours, 90), np.percentile(theirs, 90))
        if name == "icub":
            assert np.median(ours) < 1e-6, np.median(ours)


def test_contacts_are_exercised(models):
    """The contact configurations used above really have points in and out of contact."""
    for name in ("box", "anymal", "icub"):
        d = models.random_data(name, 32, seed=4)
        p, _ = oracle.collidable_points_pos_vel(models(name), link_transforms=d.link_transforms, link_velocities=d.link_velocities)
        assert (p[..., 2] < 0).any() and (p[..., 2] > 0).any()


@pytest.mark.parametrize("name", ["chain9f", "icub"])
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed])
def test_step_link_force_representations(models, name, rep):
    model = models(name)
    N = 4
    d = models.random_data(name, N, seed=8, rep=rep)
    tau, f = helpers.random_inputs(model, N, 9, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T,
                 link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[rep])  # fmt: skip
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


@pytest.mark.parametrize("name", ["cartpole", "anymal", "icub"])
def test_multi_step_rollout(models, name):
    model = models(name)
    N = 3
    d = models.random_data(name, N, seed=12)
    blk = helpers.odata_to_block(model, d)
    for _ in range(25):
        d = oracle.step(model, d)
        blk = eb.run(model, eb.MODE_STEP, blk)
    assert helpers.rel_err(blk, helpers.odata_to_block(model, d)) < 1e-8


def test_null_inputs_equal_zero_inputs(models):
    model = models("icub")
    d = models.random_data("icub", 3, seed=1)
    blk = helpers.odata_to_block(model, d)
    a = eb.run(model, eb.MODE_STEP, blk)
    b = eb.run(model, eb.MODE_STEP, blk, tau=np.zeros((model.dofs(), 3)), link_forces=np.zeros((24 * 6, 3)), force_repr=2)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["double_pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_forward_dynamics_matches_oracle(models, name, dtype):
    model = models(name)
    N = 5
    d = models.random_data(name, N, seed=6, dtype=dtype, rep=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, N, 7, dtype)
    vd, sdd = oracle.forward_dynamics_aba(model, helpers.upcast(d), joint_forces=tau.astype(np.float64), link_forces=f.astype(np.float64))
    out = eb.run(model, eb.MODE_FD, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=0)
    assert helpers.rel_err(out.T, np.concatenate([vd, sdd], -1)) < helpers.tol_of(dtype, name, evaluation=True)


@pytest.mark.parametrize("name", ["double_pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_inverse_dynamics_matches_oracle(models, name, dtype):
    model = models(name)
    N = 5
    d = models.random_data(name, N, seed=16, dtype=dtype, rep=VelRepr.Inertial)
    _, f = helpers.random_inputs(model, N, 17, dtype)
    rng = np.random.default_rng(3)
    acc = rng.uniform(-2, 2, size=(N, 6 + model.dofs())).astype(dtype)
    a64 = acc.astype(np.float64)
    fB, tau = oracle.inverse_dynamics(model, helpers.upcast(d), joint_accelerations=a64[:, 6:], base_acceleration=a64[:, :6],
                                      link_forces=f.astype(np.float64))
    out = eb.run(model, eb.MODE_ID, helpers.odata_to_block(model, d), link_forces=f.reshape(N, -1).T, force_repr=0, in_acc=acc.T)
    ref = np.concatenate([fB, tau], -1)
    if not model.floating_base():
        ref[:, :6] = out.T[:, :6]  # base wrench of a fixed base is not part of the contract (always 0 in the reference)
        assert np.all(out.T[:, :6] == 0)
    # forces scale with the inertia: compare relative to the largest entry
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(out.T - ref).max()) / scale < helpers.tol_of(dtype, name, evaluation=True)


def test_bias_forces_null_acceleration(models):
    model = models("icub")
    d = models.random_data("icub", 4, seed=21, rep=VelRepr.Inertial)
    h = oracle.free_floating_bias_forces(model, d)
    out = eb.run(model, eb.MODE_ID, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out.T, h) < helpers.FP64_TOL


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "chain5", "chain9f", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cached_kinematics_match_oracle(models, name, dtype):
    model = models(name)
    N, nL = 4, model.number_of_links()
    d = models.random_data(name, N, seed=31, dtype=dtype)
    H, V = eb.run(model, eb.MODE_KIN, helpers.odata_to_block(model, d))
    H = H.T.reshape(N, nL, 3, 4)
    d = helpers.upcast(d).update_caches(model)
    assert helpers.rel_err(H, d.link_transforms[:, :, :3, :]) < helpers.tol_of(dtype, name, evaluation=True)
    assert helpers.rel_err(V.T.reshape(N, nL, 6), d.link_velocities) < helpers.tol_of(dtype, name, evaluation=True)


def test_far_from_origin_is_well_conditioned(models):
    """Frame C is centred on the base: a robot 1 km from the world origin loses no accuracy
    in fp32 beyond what its stored inertial-fixed velocity already carries."""
    model = models("icub")
    N = 4
    d64 = models.random_data("icub", N, seed=41, dtype=np.float64, in_contact=False)
    d64.base_position[:, 0] += 1000.0
    d64.base_linear_velocity[:] = 0
    d64.base_angular_velocity[:] = 0
    d64 = d64.update_caches(model)
    ref = oracle.forward_dynamics_aba(model, dataclasses.replace(d64, velocity_representation=VelRepr.Inertial))
    blk32 = helpers.odata_to_block(model, d64, np.float32)
    out = eb.run(model, eb.MODE_FD, blk32)
    assert helpers.rel_err(out.T[:, 6:], ref[1]) < 5e-3  # joint accelerations stay accurate


def test_disabled_points_keep_their_state(models):
    model = helpers.enable_points(models("box"), [0, 1, 2, 3])
    d = models.random_data("box", 4, seed=3)
    ref = oracle.step(model, d)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL
    L = eb.layout(model)
    np.testing.assert_array_equal(out[L.row_m + 12 :], helpers.odata_to_block(model, d)[L.row_m + 12 :])


def test_non_default_contact_exponents(models):
    import jaxsim_amd as ja

    model = helpers.with_params(models("anymal"), contact_params=ja.SoftContactsParams.build(K=2e5, D=800, mu=0.8, p=0.7, q=0.4))
    d = models.random_data("anymal", 6, seed=13)
    ref = oracle.step(model, d)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


def test_unsupported_models_are_rejected(models):
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    big = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(70, fixed_base=True, seed=0))
    with pytest.raises(RuntimeError, match="64 links"):
        eb.layout(big)


@pytest.mark.parametrize("name", ["cartpole", "chain9f", "anymal", "icub"])
def test_fused_rollout_equals_repeated_steps(models, name):
    """n_steps fused in one launch (state carried in registers) == n_steps single-step launches."""
    model = models(name)
    d = models.random_data(name, 3, seed=14)
    tau, f = helpers.random_inputs(model, 3, 15, np.float64)
    blk = helpers.odata_to_block(model, d)
    kw = dict(tau=tau.T, link_forces=f.reshape(3, -1).T, force_repr=2)
    fused = eb.run(model, eb.MODE_STEP, blk, n_steps=7, **kw)
    for _ in range(7):
        blk = eb.run(model, eb.MODE_STEP, blk, **kw)
    np.testing.assert_array_equal(fused, blk)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_plane_terrain(models, dtype):
    """PlaneTerrain: tilted ground plane through the soft-contact model."""
    import jaxsim_amd as ja

    terrain = ja.PlaneTerrain.build(height=0.02, normal=[0.15, -0.1, 1.0])
    for name in ("box", "icub"):
        model = helpers.with_params(models(name), terrain=terrain)
        d = models.random_data(name, 8, seed=23, dtype=dtype)
        ref = oracle.step(model, helpers.upcast(d))
        out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
        assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype)
        # the tilted plane really changes the answer
        flat = eb.run(models(name), eb.MODE_STEP, helpers.odata_to_block(model, d))
        assert helpers.rel_err(flat, helpers.odata_to_block(model, ref)) > 1e-6


def test_plane_terrain_box_slides_downhill(models):
    """Known answer: a box at rest on a frictionless 10-degree incline accelerates at g sin(a) along it."""
    import jaxsim_amd as ja

    a = np.deg2rad(10.0)
    terrain = ja.PlaneTerrain.build(normal=[np.sin(a), 0.0, np.cos(a)])
    params = ja.SoftContactsParams.build(K=2e4, D=300.0, mu=0.0)
    model = helpers.enable_points(helpers.with_params(models("box"), terrain=terrain, contact_params=params), [0, 1, 2, 3])
    # start resting on the plane: base tilted with the plane, bottom face 0.4 mm inside
    q = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])  # rotation about +y by a: body z -> plane normal
    n = np.array([np.sin(a), 0.0, np.cos(a)])
    d = oracle.OracleData.build(model, base_position=n * (0.05 - 4e-4), base_quaternion=q)
    blk = helpers.odata_to_block(model, d)
    for _ in range(300):
        blk = eb.run(model, eb.MODE_STEP, blk)
        d = oracle.step(model, d)
    assert helpers.rel_err(blk, helpers.odata_to_block(model, d)) < 1e-8
    t = 0.3
    downhill = np.array([np.cos(a), 0.0, -np.sin(a)])
    travelled = float(blk[0:3, 0] @ downhill - (n * (0.05 - 4e-4)) @ downhill)
    assert travelled == pytest.approx(0.5 * 9.81 * np.sin(a) * t * t, rel=0.03)


# ---- Runge-Kutta 4 (reference: api/integrators.py:91-167; the softer ground: pc.rk4) ----
@pytest.mark.parametrize("name", RK4_MODELS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rk4_step_matches_oracle(models, name, dtype):
    model = pc.rk4(models(name))
    N = 5
    d = models.random_data(name, N, seed=31, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 32, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T,
                 link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[d.velocity_representation])  # fmt: skip
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    # and it is not the Euler answer
    euler = oracle.step(helpers.with_params(model, integrator=0), helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    assert helpers.rel_err(helpers.odata_to_block(model, euler), helpers.odata_to_block(model, ref)) > 1e-7


@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed])
def test_rk4_link_forces_are_held_over_the_stages(models, rep):
    """The external wrenches are converted to inertial once, with the link transforms of the
    initial state (api/model.py:2641-2646), and held while the stages move the links."""
    model = pc.rk4(models("chain9f"))
    N = 4
    d = models.random_data("chain9f", N, seed=33, rep=rep)
    tau, f = helpers.random_inputs(model, N, 34, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T,
                 link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[rep])  # fmt: skip
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


def test_rk4_multi_step_rollout(models):
    for name in ("cartpole", "icub16"):
        model = pc.rk4(models(name))
        d = models.random_data(name, 3, seed=35)
        blk = helpers.odata_to_block(model, d)
        for _ in range(10):
            d = oracle.step(model, d)
        out = eb.run(model, eb.MODE_STEP, blk, n_steps=10)  # one launch per step
        assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8


def test_rk4_free_fall_known_answer(models):
    """Constant acceleration: RK4 integrates position exactly, p(t) = p0 + v0 t + g t^2 / 2
    (semi-implicit Euler has an O(dt) position error on the same problem)."""
    model = pc.rk4(models("box"))
    v0 = np.array([0.3, -0.2, 1.0])
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 5.0], base_linear_velocity=v0)
    blk = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), n_steps=50)
    t = 50 * model.time_step
    expect = np.array([0.0, 0.0, 5.0]) + v0 * t + 0.5 * np.array([0.0, 0.0, model.gravity]) * t * t
    np.testing.assert_allclose(blk[0:3, 0], expect, rtol=0, atol=1e-12)


def test_rk4_pendulum_energy_drift_is_fourth_order(models):
    """Undamped pendulum: the RK4 energy drift over 200 steps is orders of magnitude below
    semi-implicit Euler's bounded oscillation at the same time step."""
    import jaxsim_amd as ja

    base = helpers.with_params(models("pendulum"), actuation_params=ja.ActuationParams(enable_friction=False))

    def energy(model, blk):
        dd = helpers.block_to_odata(model, blk)
        M = oracle.free_floating_mass_matrix(model, dd)
        v = dd.generalized_velocity(VelRepr.Inertial) if model.floating_base() else np.concatenate([np.zeros((1, 6)), dd.joint_velocities], -1)
        T = 0.5 * np.einsum("ni,nij,nj->n", v, M, v)
        H = dd.link_transforms
        kdp = model.kin_dyn_parameters
        com_w = np.einsum("nlij,lj->nli", H[:, :, :3, :3], kdp.link_com) + H[:, :, :3, 3]
        U = -model.gravity * np.einsum("l,nl->n", kdp.link_mass, com_w[..., 2])
        return (T + U)[0]

    out = {}
    for key, model in (("euler", base), ("rk4", pc.rk4(base))):
        d = oracle.OracleData.build(model, joint_positions=[1.0])
        blk = helpers.odata_to_block(model, d)
        e0 = energy(model, blk)
        drift = 0.0
        for _ in range(4):
            blk = eb.run(model, eb.MODE_STEP, blk, n_steps=50)
            drift = max(drift, abs(energy(model, blk) - e0))
        out[key] = drift / abs(e0) if e0 != 0 else drift
    assert out["rk4"] < 1e-9 and out["rk4"] < 1e-3 * out["euler"], out


def test_config1_double_pendulum_from_sdf(models):
    """BASELINE.json configs[0]: 2-link pendulum, fixed base, no contacts, batch 1, fp64 -- built from
    the SDF form of the model (the reference's fixture is an SDF file) and stepped against the oracle."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    model = ja.JaxSimModel.build_from_model_description(robots.double_pendulum_sdf())
    d = oracle.random_model_data(model, batch_size=1, seed=3)
    tau = np.array([[0.3, -0.2]])
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, n_steps=1)
    ref = oracle.step(model, d, joint_force_references=tau)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL
    # and it is the same model as the URDF form used everywhere else in the tests
    ref_urdf = oracle.step(models("double_pendulum"), d, joint_force_references=tau)
    np.testing.assert_allclose(helpers.odata_to_block(model, ref), helpers.odata_to_block(models("double_pendulum"), ref_urdf), atol=1e-12)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-4)])
def test_rk4_with_more_points_than_lanes(models, dtype, tol):
    """[round 4] RungeKutta4 with several chunks of collidable points (SoftContacts): the points behind the first
    chunk go through memory at every stage, their stage data (rate of the previous stage, weighted sum of the rates)
    sit in the LDS (jxs_core.h contact_chunk).  80 points on a 24-link humanoid: 32 lanes, three chunks.  Against the
    oracle, one step and a short rollout (in place: the deformation rows are read at every stage and written at the last)."""
    model = pc.rk4(pc.icub80())
    lay = eb.layout(model)
    assert lay.group == 32 and lay.n_points == 80
    N = 6
    d = pc.icub80_data(model, N, dtype)
    rng = np.random.default_rng(5)
    d.tangential_deformation[:] = (1e-3 * rng.normal(size=d.tangential_deformation.shape)).astype(dtype)
    tau, f = helpers.random_inputs(model, N, 7, dtype)
    kw = dict(link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    ref = oracle.step(model, helpers.upcast(d), **kw)
    blk = helpers.odata_to_block(model, d)
    run = dict(tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[d.velocity_representation])
    out = eb.run(model, eb.MODE_STEP, blk, **run)
    truth = helpers.odata_to_block(model, ref)
    assert helpers.rel_err(out, truth) < tol
    # the deformation rows of the LAST chunk moved, and not by the Euler rule
    lay_rows = slice(truth.shape[0] - 3 * 16, truth.shape[0])
    assert np.abs(out[lay_rows] - blk[lay_rows]).max() > 0
    euler = helpers.odata_to_block(model, oracle.step(helpers.with_params(model, integrator=0), helpers.upcast(d), **kw))
    assert helpers.rel_err(euler, truth) > 1e-7
    if dtype == np.float64:
        ref3 = helpers.upcast(d)
        for _ in range(3):
            ref3 = oracle.step(model, ref3, **kw)
        out3 = eb.run(model, eb.MODE_STEP, blk, n_steps=3, **run)
        assert helpers.rel_err(out3, helpers.odata_to_block(model, ref3)) < 1e-9


def test_rk4_point_limits(models):
    """One lane per point up to 64 points (a group of 64 lanes), chunks beyond; the rigid contact models and an LDS
    budget still bound RungeKutta4 (documented limits, rejected at model creation)."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    mid = ja.JaxSimModel.build_from_model_description(robots.icub23_urdf(sole_boxes_per_foot=3))  # 48 points
    assert eb.layout(mid).group == 32 and eb.layout(pc.rk4(mid)).group == 64  # RK4: one lane per point
    big = pc.icub80()
    assert eb.layout(big).n_points > 64 and eb.layout(pc.rk4(big)).group == 32  # three chunks of 32
    rigid = helpers.with_params(helpers.rigid_model(big, list(range(80)), K=1e4, D=2e2), integrator=ja.IntegratorType.RungeKutta4)
    with pytest.raises(RuntimeError, match="one lane group"):
        eb.layout(rigid)
    with pytest.raises(RuntimeError, match="unsupported integrator"):
        eb.layout(helpers.with_params(models("box"), integrator=7))


# ---- RigidContacts (the cases: parity_cases.RIGID_CASES) -------
@pytest.mark.parametrize("key", list(RIGID_CASES))
def test_rigid_step_matches_oracle(models, reduced_qp, key):
    model, d = pc.rigid_case(models, key, 8, seed=5)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=2)
    # 1e-7: the Delassus matrix of several points on one rigid foot is singular up to the 1e-6 shift
    # (condition ~1e7), rounding differences are amplified by it
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < 1e-7
    # contacts really act in this sample
    pb = reduced_qp.rigid_problem(model, d)
    assert (~pb["inactive"]).any()


@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body])
def test_rigid_link_force_representations(models, reduced_qp, rep):
    model, d = pc.rigid_case(models, "anymal4", 4, seed=9, rep=rep)
    tau, f = helpers.random_inputs(model, 4, 10, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(4, -1).T, force_repr=REPR_CODE[rep])
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < 1e-9


def test_rigid_tight_solver_tolerance_is_statement_independent(models):
    """With solver_tol = 1e-10 the kernel (reduced QP) and the reference's statement of the QP
    converge to the same, unique, minimiser."""
    model, d = pc.rigid_case(models, "anymal4", 6, seed=5, build=dict(solver_options={"solver_tol": 1e-10}))
    ref = oracle.step(model, d)  # reference form (REDUCED_QP off)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < 1e-8


@pytest.mark.parametrize("key,tol", [("box4", 3e-3), ("anymal4", 3e-3), ("icub8", 3e-3)])
def test_rigid_step_fp32(models, reduced_qp, key, tol):
    """fp32 against the fp64 oracle on the same inputs, well-conditioned contact sets (one point per
    rigid body in contact or a single box)."""
    model, d = pc.rigid_case(models, key, 8, seed=5, dtype=np.float32)
    ref = oracle.step(model, helpers.upcast(d))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert out.dtype == np.float32
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < tol


def test_rigid_tumbling_box_rollout(models, reduced_qp):
    """300 steps of a box dropped on an edge with forward speed: impacts, sliding, rolling."""
    model, d = pc.tumbling_box(models, "rigid")
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), n_steps=300)
    for _ in range(300):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8
    assert d.base_position[0, 2] < 0.06  # it landed


@pytest.mark.parametrize("dtype,atol", [(np.float64, 1e-4), (np.float32, 2e-4)])
def test_rigid_box_settles_known_answer(models, dtype, atol):
    """reference tests/test_simulations.py:245-292: z -> box_height / 2 = 0.05 with no penetration."""
    model = pc.settling_box(models, "rigid")
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d).astype(dtype), n_steps=1000)
    assert abs(out[0, 0]) < 1e-6 and abs(out[1, 0]) < 1e-6
    assert out[2, 0] == pytest.approx(0.05, abs=atol)


# ---- RelaxedRigidContacts (the cases: parity_cases.RELAXED_CASES) ----
@pytest.mark.parametrize("key", list(RELAXED_CASES))
def test_relaxed_step_matches_oracle(models, key):
    model, d = pc.relaxed_case(models, key, 16, seed=5)
    tau, f = helpers.random_inputs(model, 16, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(16, -1).T, force_repr=2)
    # box4 / icub16d keep the default mu = 0.005: the regulariser is ~1e-6 of the Delassus entries
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-9 if key in ("box4", "icub16d") else 1e-11)
    from oracle import refrelaxed

    assert refrelaxed.relaxed_problem(model, d)["active"].any()


def test_relaxed_defaults_in_fp32_stay_finite(models):
    """[round 4] The reference's default RelaxedRigidContacts parameters (mu = 0.005) in fp32 with every sole point of the
    humanoid active (a Delassus matrix of rank 12 in 96 unknowns, the regulariser below its fp32 rounding): pivots at the
    rounding floor are dropped and the refinement is safeguarded (jxs_rigid.inc relaxed_contact_forces) -- finite states
    a few per cent from fp64, where rounds 1-3 returned NaN; fp64 is solved in the tree and is exact."""
    model = helpers.relaxed_model(models("icub"), list(range(32)))
    d32 = helpers.standing_data(model, 12, seed=0, dtype=np.float32, noise=0.003)
    truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32)))
    out32 = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d32))
    assert np.isfinite(out32).all() and helpers.rel_err(out32, truth) < 0.3
    d64 = helpers.standing_data(model, 12, seed=0, noise=0.003)
    out64 = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d64))
    assert helpers.rel_err(out64, helpers.odata_to_block(model, oracle.step(model, d64))) < 1e-10


@pytest.mark.parametrize("key,tol", [("box8", 2e-5), ("anymal16", 2e-5), ("anymal4", 2e-5), ("chain9f6", 1e-4), ("icub16", 2e-4), ("box4", 1e-1)])
def test_relaxed_step_fp32(models, key, tol):
    """fp32 kernel arithmetic against the fp64 oracle on the same (fp32-representable) inputs.  box4 runs
    the bare default mu = 0.005: the regulariser sits at the fp32 rounding level of the Delassus entries
    (condition ~1e6..1e7), the result is noise-limited at 1e-2 .. 1e-1 whatever the solver does -- the fp32
    NumPy restatement is 3e-2 away from fp64 there (HISTORY.md section 4e: use fp64 or the estimated
    parameters, mu = 0.5, with fp32)."""
    model, d32 = pc.relaxed_case(models, key, 16, seed=5, dtype=np.float32)
    tau, f = helpers.random_inputs(model, 16, 7, np.float32)
    blk = helpers.odata_to_block(model, d32)
    d64 = helpers.block_to_odata(model, blk.astype(np.float64), oracle.VelRepr.Mixed)
    ref = oracle.step(model, d64, link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = eb.run(model, eb.MODE_STEP, blk, tau=tau.T, link_forces=f.reshape(16, -1).T, force_repr=2)
    assert out.dtype == np.float32
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < tol


@pytest.mark.parametrize("kind,name,idx,dtype,tol", [
    ("relaxed", "icub", list(range(32)), np.float64, 1e-11),
    ("relaxed", "icub", list(range(32)), np.float32, 5e-5),
    ("relaxed", "anymal", helpers.ANYMAL_FEET_16, np.float32, 5e-5),
    ("rigid", "icub", list(range(32)), np.float64, 1e-7),
])  # fmt: skip
def test_standing_on_every_sole_point(models, reduced_qp, kind, name, idx, dtype, tol):
    """Standing states: every bottom point of every foot in contact (16 active points; the 32-point
    humanoid is BASELINE.json config 3's model with all its points enabled).  The Delassus matrix has
    rank <= 18 of 48.  RigidContacts is checked on the humanoid in fp64 only.  The quadruped standing on
    straight legs is left out for that model: the stance is a kinematic singularity, the contact Jacobian
    has a singular value at 1e-7 .. 1e-14 of the largest (measured), and whether the impact removes the
    velocity along it is decided by the rcond of the reference's SVD -- a knife edge, not a parity
    statement (HISTORY.md section 4d); in fp32 that direction is below the rounding level altogether."""
    model, d = pc.standing_case(models, kind, name, idx, 6, dtype)
    blk = helpers.odata_to_block(model, d)
    d64 = helpers.block_to_odata(model, blk.astype(np.float64), oracle.VelRepr.Mixed)
    from oracle import refrigid

    assert ((~refrigid.rigid_problem(model, d64)["inactive"]).sum(axis=1) == 16).all()
    ref = oracle.step(model, d64)
    out = eb.run(model, eb.MODE_STEP, blk)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < tol


def test_relaxed_tumbling_box_rollout(models):
    """300 steps of a box dropped on an edge with forward speed."""
    model, d = pc.tumbling_box(models, "relaxed")
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), n_steps=300)
    for _ in range(300):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8
    assert d.base_position[0, 2] < 0.08  # it landed


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relaxed_box_settles_known_answer(models, dtype):
    """reference tests/test_simulations.py:295-346: x, y unchanged (atol 1e-5), z -> 0.05 (atol 1e-4)."""
    model = pc.settling_box(models, "relaxed")
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d).astype(dtype), n_steps=1000)
    assert abs(out[0, 0]) < 1e-5 and abs(out[1, 0]) < 1e-5
    assert out[2, 0] == pytest.approx(0.05, abs=1e-4)


def test_relaxed_unsupported_configurations_are_rejected(models):
    import jaxsim_amd as ja

    # [round 3] up to 64 enabled points (one lane each): the 50-point sphere is accepted
    assert eb.layout(helpers.relaxed_model(models("sphere"), list(range(50)))).group == 64
    with pytest.raises(RuntimeError, match="RelaxedRigidContactsParams"):
        eb.layout(helpers.relaxed_model(models("box"), [0, 1, 2, 3], time_constant=0.0))


@pytest.mark.parametrize("key", ["box8", "anymal16", "chain9f6", "icub16"])
def test_relaxed_rk4_step_matches_oracle(models, key):
    """RungeKutta4 with RelaxedRigidContacts: the contact forces are solved at each of the four stages
    (api/integrators.py:91-167 calls system_dynamics -> system_acceleration -> link_contact_forces per
    stage); the reference runs its relaxed-rigid test for every integrator (tests/test_simulations.py:295)."""
    import jaxsim_amd as ja

    model, d = pc.relaxed_case(models, key, 8, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    euler = oracle.step(helpers.with_params(model, integrator=ja.IntegratorType.SemiImplicitEuler), d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=2)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < 1e-10
    assert helpers.rel_err(helpers.odata_to_block(model, euler), helpers.odata_to_block(model, ref)) > 1e-6  # a different integrator


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relaxed_rk4_box_settles_known_answer(models, dtype):
    """reference tests/test_simulations.py:295-346 with integrator = RungeKutta4."""
    import jaxsim_amd as ja

    model = pc.settling_box(models, "relaxed", ja.IntegratorType.RungeKutta4)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d).astype(dtype), n_steps=1000)
    assert abs(out[0, 0]) < 1e-5 and abs(out[1, 0]) < 1e-5
    assert out[2, 0] == pytest.approx(0.05, abs=1e-4)


@pytest.mark.parametrize("key", ["box4", "anymal4", "chain9f6"])
def test_rigid_rk4_step_matches_oracle(models, reduced_qp, key):
    """RungeKutta4 with RigidContacts: QP forces at each stage, the impact on the integrated state
    (api/model.py:2665-2679); the reference runs its rigid-contact test for every integrator
    (tests/test_simulations.py:245)."""
    import jaxsim_amd as ja

    model, d = pc.rigid_case(models, key, 8, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=2)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < 1e-7


@pytest.mark.parametrize("dtype,atol", [(np.float64, 1e-4), (np.float32, 2e-4)])
def test_rigid_rk4_box_settles_known_answer(models, dtype, atol):
    """reference tests/test_simulations.py:245-292 with integrator = RungeKutta4."""
    import jaxsim_amd as ja

    model = pc.settling_box(models, "rigid", ja.IntegratorType.RungeKutta4)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d).astype(dtype), n_steps=1000)
    assert abs(out[0, 0]) < 1e-6 and abs(out[1, 0]) < 1e-6
    assert out[2, 0] == pytest.approx(0.05, abs=atol)


@pytest.mark.parametrize("kind,key", [("relaxed", "box8"), ("relaxed", "anymal16"), ("relaxed", "chain9f6"), ("rigid", "box4"), ("rigid", "anymal4")])
def test_rk4fast_step_matches_oracle(models, reduced_qp, kind, key):
    """RungeKutta4Fast (api/integrators.py:170-276) with the contact models without contact state: contact
    forces once, position derivatives of the initial data at every stage -- restated as written in
    oracle/refstep.py::rk4fast_integration.  The reference runs its rigid / relaxed-rigid tests with this
    integrator too (tests/conftest.py:148-152)."""
    import jaxsim_amd as ja

    model, d = pc.contact_case(models, kind, key, 8, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4Fast)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    rk4 = oracle.step(helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4), d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=2)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-10 if kind == "relaxed" else 1e-7)
    assert helpers.rel_err(helpers.odata_to_block(model, rk4), helpers.odata_to_block(model, ref)) > 1e-7  # not RungeKutta4


def test_rk4fast_relaxed_box_settles_known_answer(models):
    """reference tests/test_simulations.py:295-346 with integrator = RungeKutta4Fast."""
    import jaxsim_amd as ja

    model = pc.settling_box(models, "relaxed", ja.IntegratorType.RungeKutta4Fast)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), n_steps=1000)
    assert abs(out[0, 0]) < 1e-5 and abs(out[1, 0]) < 1e-5
    assert out[2, 0] == pytest.approx(0.05, abs=1e-4)


def test_rk4fast_rigid_box_rollout_keeps_its_landing_penetration(models, reduced_qp):
    """RungeKutta4Fast as written advances the positions with the velocities of the *initial* data of the
    step (integrators.py:200-203).  With RigidContacts the impact zeroes the velocity of a resting box
    after every step, so the Baumgarte correction never reaches the position: the box keeps the penetration
    it landed with instead of returning to z = 0.05 (the restatement and the kernel agree on that; whether
    the reference's own rigid-contact test passes with this integrator cannot be checked here)."""
    import jaxsim_amd as ja

    model = pc.settling_box(models, "rigid", ja.IntegratorType.RungeKutta4Fast)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.06], velocity_representation=VelRepr.Inertial)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), n_steps=200)
    for _ in range(200):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-7
    assert 0.05 - 2e-3 < out[2, 0] < 0.05 - 1e-5


def test_rk4fast_is_refused_where_the_reference_is_broken(models):
    """SoftContacts (the tangential deformation is overwritten by its derivative, integrators.py:189-191,
    214, 225) and models without collidable points (NameError, :175-187)."""
    import jaxsim_amd as ja

    with pytest.raises(RuntimeError, match="RungeKutta4Fast"):
        eb.layout(helpers.with_params(models("box"), integrator=ja.IntegratorType.RungeKutta4Fast))
    with pytest.raises(RuntimeError, match="RungeKutta4Fast"):
        eb.layout(helpers.with_params(models("cartpole"), integrator=ja.IntegratorType.RungeKutta4Fast))
    with pytest.raises(NotImplementedError):
        oracle.step(helpers.with_params(models("box"), integrator=ja.IntegratorType.RungeKutta4Fast), models.random_data("box", 1))


def test_rigid_unsupported_configurations_are_rejected(models, monkeypatch):
    import jaxsim_amd as ja

    # up to 64 enabled points.  [round 4] The 50-point sphere of the reference in fp64 -- refused in round 3: the two
    # triangles of RigidContacts are 182 KB, more than the LDS of a CU -- is accepted: in fp64 the contact problem is
    # solved in the tree, without any triangle (jxs_rigid.inc ta_*; round 4: link space).  The dense path still says why
    # it cannot take it (the developer knob switches the tree solve off).
    assert eb.layout(helpers.rigid_model(models("sphere"), list(range(50))), np.float64).group == 64
    monkeypatch.setenv("JXS_DISABLE_CT_TREE", "1")
    with pytest.raises(RuntimeError, match="does not fit"):
        eb.layout(helpers.rigid_model(models("sphere"), list(range(50))), np.float64)
    monkeypatch.delenv("JXS_DISABLE_CT_TREE")
    assert eb.layout(helpers.rigid_model(models("sphere"), list(range(50))), np.float32).group == 64
    # [round 3] fixed-base models are accepted (test_fixed_base_rigid_contacts_match_oracle)
    fixed = ja.JaxSimModel.build_from_model_description(ja.robots.cartpole_urdf(with_collisions=True))
    assert eb.layout(helpers.rigid_model(fixed, [0, 1, 2, 3])).group >= 4


@pytest.mark.parametrize("kind,key,dtype,tol", [
    ("relaxed", "icub16", np.float64, 1e-11), ("relaxed", "icub16", np.float32, 2e-4), ("relaxed", "serial12f", np.float64, 1e-11),
    ("relaxed", "icub16d", np.float64, 1e-9),  # default parameters (mu = 0.005): in the tree in fp64 only
    ("relaxed", "serial12f", np.float32, 2e-3), ("rigid", "icub8", np.float64, 1e-7), ("rigid", "serial12f", np.float64, 1e-7),
    # [round 5] what link space could not take: parallel joint axes between the contact links, four contact links
    ("relaxed", "planar_biped", np.float64, 1e-11), ("relaxed", "planar_biped", np.float32, 2e-4), ("rigid", "planar_biped", np.float64, 1e-7),
    ("relaxed", "planar10f", np.float64, 1e-11), ("relaxed", "planar10f", np.float32, 2e-3), ("rigid", "planar10f", np.float64, 1e-7),
    ("relaxed", "anymal16", np.float64, 1e-11), ("relaxed", "anymal16", np.float32, 2e-4), ("rigid", "anymal16", np.float64, 1e-7),
])  # fmt: skip
def test_tree_solve_agrees_with_the_dense_path(models, reduced_qp, kind, key, dtype, tol, monkeypatch):
    """[round 5] The systems (J M^-1 J^T + D) x = c of the contact models are solved IN THE TREE (jxs_rigid.inc ta_*: a
    forward-dynamics solve of the tree with W = P^T D^-1 P added to the inertia of the contact links -- no matrix, no
    rank decision, any number of contact links); the developer knob switches back to the packed triangles in the LDS.
    Both paths against the oracle within the stated tolerance, and within it of each other; the kernel description says
    which path a model takes.  (Round 4 solved these in link space through a Cholesky factor of the 12 x 12 B of at most
    two links, which is singular between parallel-axis joints: the planar cases here are the ones it got wrong.)"""
    from jaxsim_amd import specialize

    model, d = pc.contact_case(models, kind, key, 16, seed=5, dtype=dtype)
    truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d) if dtype == np.float32 else d))
    blk = helpers.odata_to_block(model, d)
    if kind == "rigid":
        # RigidContacts takes the tree only where the triangles do not fit the LDS (jxs_pack.h: its Newton directions are
        # fragile near convergence); the developer knob runs it wherever it applies
        assert "P.ct_tree=0" in specialize.spec(model, dtype, specialize.MODE_STEP_RIGID)
        monkeypatch.setenv("JXS_CT_TREE_RIGID", "1")
    assert "P.ct_tree=1" in specialize.spec(model, dtype, specialize.MODE_STEP_RIGID)
    tree = eb.run(model, eb.MODE_STEP, blk)
    monkeypatch.setenv("JXS_DISABLE_CT_TREE", "1")
    assert "P.ct_tree=0" in specialize.spec(model, dtype, specialize.MODE_STEP_RIGID)
    dense = eb.run(model, eb.MODE_STEP, blk)
    assert helpers.rel_err(tree, truth) < tol and helpers.rel_err(dense, truth) < tol
    assert helpers.rel_err(tree, dense) < 2 * tol and not np.array_equal(tree, dense)
    # RigidContacts in fp32 and at tight solver tolerances keeps the triangles (jxs_pack.h: the cancellation in c - J a)
    monkeypatch.delenv("JXS_DISABLE_CT_TREE")
    if key == "icub16d":  # fp32 keeps the triangles at the bare defaults
        assert "P.ct_tree=0" in specialize.spec(model, np.float32, specialize.MODE_STEP_RIGID)
    if kind == "rigid":
        assert "P.ct_tree=0" in specialize.spec(model, np.float32, specialize.MODE_STEP_RIGID)
        name, idx, params = RIGID_CASES[key]
        tight = helpers.rigid_model(models(name), idx, build=dict(solver_options={"solver_tol": 1e-10}), **params)
        assert "P.ct_tree=0" in specialize.spec(tight, np.float64, specialize.MODE_STEP_RIGID)


@pytest.mark.parametrize("name,dtype,tol", [("planar_biped", np.float32, 3e-4), ("planar10f", np.float32, 3e-3), ("planar_biped", np.float64, 1e-10)])
def test_parallel_axis_models_with_relaxed_contacts(models, name, dtype, tol):
    """[round 5, VERDICT r4 weak #1] Contact links joined by PARALLEL joint axes -- a planar biped (torso + 2 x thigh /
    shank / foot, six pitch joints), a planar serial chain: round 4's link-space solve factorised a 12 x 12 matrix that is
    singular for them in every configuration and returned fp32 steps wrong by up to 124 % in 2 % of the states.  Random
    and standing states against the fp64 oracle; the campaign of profiles/r05_parallel_axes.txt ran 10 000 states."""
    model = helpers.relaxed_model(models(name), list(range(16)), mu=0.5)
    worst = 0.0
    for seed in (0, 1):
        for d in (models.random_data(name, 128, seed=seed, dtype=dtype), helpers.standing_data(model, 128, seed=seed, dtype=dtype, noise=0.3)):
            truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d, model) if dtype == np.float32 else d))
            out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
            worst = max(worst, helpers.rel_err(out, truth))
    helpers.note(f"parallel_axes/{name}/{np.dtype(dtype).name}", worst)
    assert worst < tol


@pytest.mark.parametrize("name,kind", [("icub16", "euler"), ("cartpole", "euler"), ("double_pendulum", "euler"), ("chain9f", "rk4"), ("anymal", "rigid"), ("icub80", "euler")])
def test_controlled_rollout_equals_the_step_loop(models, name, kind):
    """[round 4] jxs_rollout_controlled: K steps with a torque SEQUENCE [K * n][N] (what jax.lax.scan over step with
    precomputed joint_force_references does) -- one fused launch with a torque load per step where the steps fuse
    (semi-implicit Euler, SoftContacts, one point chunk), one launch per step with the step's rows gathered otherwise
    (RungeKutta4, RigidContacts, several chunks: icub80).  Against the oracle stepping with tau[k], and not equal to
    the rollout that holds tau[0]."""
    K, N = 4, 5
    model, d = pc.rollout_case(models, name, kind, N, seed=21)
    n = model.dofs()
    rng = np.random.default_rng(11)
    tau = rng.uniform(-3, 3, size=(K, N, n))
    ref = d
    for k in range(K):
        ref = oracle.step(model, ref, joint_force_references=tau[k])
    blk = helpers.odata_to_block(model, d)
    seq = np.ascontiguousarray(tau.transpose(0, 2, 1).reshape(K * n, N))
    out = eb.run(model, eb.MODE_STEP, blk, tau=seq, n_steps=K, tau_seq=True, force_repr=2)
    # (RigidContacts at the default solver_tol = 1e-3: four steps agree to the tolerance of the QP iterates)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-5 if kind == "rigid" else 1e-9)
    held = eb.run(model, eb.MODE_STEP, blk, tau=np.ascontiguousarray(tau[0].T), n_steps=K, force_repr=2)
    assert helpers.rel_err(held, out) > 1e-6


@pytest.mark.parametrize("name,kind,seq", [("icub16", "euler", True), ("cartpole", "euler", False), ("chain9f", "rk4", True), ("anymal", "rigid", False), ("icub80", "euler", True), ("icub16", "disabled", True)])
def test_recorded_rollout_returns_every_step(models, name, kind, seq):
    """[round 4] jxs_rollout_recorded: the state block after EVERY step of a rollout (the stacked outputs of the
    reference's jax.lax.scan over step) -- stored from registers inside the fused launch, or copied per step where the
    steps do not fuse (RungeKutta4, RigidContacts, several point chunks, disabled points).  Every recorded state equals
    the oracle's after that many steps; the last one is the final state."""
    K, N = 4, 5
    model, d = pc.rollout_case(models, name, kind, N, seed=23)
    n = model.dofs()
    tau = np.random.default_rng(13).uniform(-3, 3, size=(K, N, n))
    if not seq:
        tau[:] = tau[0]
    blk = helpers.odata_to_block(model, d)
    arg = np.ascontiguousarray(tau.transpose(0, 2, 1).reshape(K * n, N)) if seq else np.ascontiguousarray(tau[0].T)
    final, states = eb.run(model, eb.MODE_STEP, blk, tau=arg, n_steps=K, tau_seq=seq, record=True, force_repr=2)
    assert states.shape == (K,) + blk.shape
    ref = d
    tol = 1e-5 if kind == "rigid" else 1e-9
    for k in range(K):
        ref = oracle.step(model, ref, joint_force_references=tau[k])
        assert helpers.rel_err(states[k], helpers.odata_to_block(model, ref)) < tol, k
    np.testing.assert_array_equal(states[-1], final)
    plain = eb.run(model, eb.MODE_STEP, blk, tau=arg, n_steps=K, tau_seq=seq, force_repr=2)
    np.testing.assert_array_equal(plain, final)  # recording does not change the rollout


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 3e-3)])
def test_relaxed_contacts_with_more_points_than_lanes(dtype, tol):
    """[round 5] RelaxedRigidContacts beyond 64 enabled points (missing #3): 200 points on four links in chunks of
    64 lanes, solved in the tree (jxs_rigid.inc relaxed_contact_forces_chunked) -- random states with a few points down
    and standing states, against the oracle; ten in-place steps stay on the oracle's trajectory."""
    model = helpers.relaxed_model(pc.quadruped_200(), range(200), mu=0.5)
    assert eb.layout(model, dtype).group == 64  # four chunks of a full wave (measured faster than seven of 32 lanes)
    worst = 0.0
    for d in (oracle.random_model_data(model, batch_size=12, seed=1, dtype=dtype, base_pos_bounds=((-1, -1, 0.55), (1, 1, 0.68)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3))),
              helpers.standing_data(model, 12, seed=1, dtype=dtype, noise=0.05)):  # fmt: skip
        p, _ = oracle.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
        assert (p[..., 2] < 0).any()
        truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d, model) if dtype == np.float32 else d))
        out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
        worst = max(worst, helpers.rel_err(out, truth))
    helpers.note(f"relaxed_200_points/{np.dtype(dtype).name}", worst)
    assert worst < tol
    if dtype == np.float64:
        d = helpers.standing_data(model, 3, seed=2, noise=0.05)
        ref, blk = d, helpers.odata_to_block(model, d)
        for _ in range(10):
            ref = oracle.step(model, ref)
            blk = eb.run(model, eb.MODE_STEP, blk)
        assert helpers.rel_err(blk, helpers.odata_to_block(model, ref)) < 1e-8


@pytest.mark.parametrize("n_points,lanes", [(40, 32), (65, 32), (100, 16), (32, 16)])
def test_chunked_relaxed_solve_equals_the_one_chunk_form(models, n_points, lanes, monkeypatch):
    """[round 5] The chunked form against the one-lane-per-point form of the SAME problem (a developer knob caps the lane
    group, so that up to 64 points run both ways) and against the oracle: full and partly filled last chunks, a link's
    points split over chunk borders."""
    base = pc.quadruped_200() if n_points > 32 else models("anymal")
    model = helpers.relaxed_model(base, range(n_points), mu=0.5)
    d = helpers.standing_data(model, 8, seed=1, noise=0.05)
    blk = helpers.odata_to_block(model, d)
    truth = helpers.odata_to_block(model, oracle.step(model, d))
    one = eb.run(model, eb.MODE_STEP, blk) if n_points <= 64 else None
    monkeypatch.setenv("JXS_CT_CHUNK_LANES", str(lanes))
    assert eb.layout(model).group == lanes
    chunked = eb.run(model, eb.MODE_STEP, blk)
    assert helpers.rel_err(chunked, truth) < 1e-10
    if one is not None:
        assert helpers.rel_err(chunked, one) < 1e-11


def test_rigid_contacts_fp64_beyond_47_points_on_three_links(reduced_qp):
    """[round 5] RigidContacts in the reference's default precision with 60 points on THREE links: the two triangles of the
    dense path (180 x 180 doubles twice: 260 KB) do not fit the LDS of a CU, round 4's link space took two links at most --
    refused until now.  The interior-point iteration runs in the tree (adaptive refinement of its Newton directions, best
    iterate kept: jxs_rigid.inc rigid_qp_tree), which is the path such a model takes by default."""
    from jaxsim_amd import specialize

    idx = list(range(0, 20)) + list(range(50, 70)) + list(range(100, 120))
    model = helpers.rigid_model(pc.quadruped_200(), idx, K=1e4, D=2e2)
    assert "P.ct_tree=1" in specialize.spec(model, np.float64, specialize.MODE_STEP_RIGID) and eb.layout(model, np.float64).group == 64
    with pytest.raises(RuntimeError, match="does not fit"):
        import os

        os.environ["JXS_DISABLE_CT_TREE"] = "1"
        try:
            eb.layout(model, np.float64)
        finally:
            del os.environ["JXS_DISABLE_CT_TREE"]
    for d in (oracle.random_model_data(model, batch_size=8, seed=2, base_pos_bounds=((-1, -1, 0.56), (1, 1, 0.66)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3))),
              helpers.standing_data(model, 8, seed=2, noise=0.05)):  # fmt: skip
        truth = helpers.odata_to_block(model, oracle.step(model, d))
        out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
        assert helpers.rel_err(out, truth) < 1e-6


def test_more_points_than_lanes_outside_the_tree_solve_is_refused():
    """What still needs one lane per point says so: RigidContacts, RelaxedRigidContacts in fp32 with the bare default
    regulariser (the dense path), Runge-Kutta with a rigid contact model."""
    import jaxsim_amd as ja

    base = pc.quadruped_200()
    with pytest.raises(RuntimeError, match="at most 64"):
        eb.layout(helpers.rigid_model(base, range(200)), np.float64)
    with pytest.raises(RuntimeError, match="at most 64"):
        eb.layout(helpers.relaxed_model(base, range(200)), np.float32)  # mu = 0.005: no tree solve in fp32
    assert eb.layout(helpers.relaxed_model(base, range(200)), np.float64).group == 64  # fp64: in the tree
    with pytest.raises(RuntimeError, match="RungeKutta4"):
        eb.layout(helpers.with_params(helpers.relaxed_model(base, range(200), mu=0.5), integrator=ja.IntegratorType.RungeKutta4), np.float64)


def test_contact_tree_solve_on_random_trees():
    """[round 5] Random floating trees (8 to 24 links) with the two collision boxes on random links -- neighbours, far
    apart, on the base; every third tree with all joint axes parallel, every third with axis-aligned joints: every pair
    is solved in the tree (round 4's link space took only pairs six or more joints apart, and was wrong for the parallel
    ones) and agrees with the oracle in fp64 and in fp32."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots, specialize

    rng = np.random.default_rng(7)
    worst32 = 0.0
    for trial in range(24):
        n_links = int(rng.integers(8, 25))
        seed = 100 + trial
        max_back = 1 if trial % 3 == 0 else int(rng.integers(1, 4))  # every third tree a serial chain: far-apart links
        a, b = sorted(int(v) for v in rng.choice(np.arange(0, n_links), size=2, replace=False))
        axes = [None, "all", "aligned"][(trial // 3) % 3]
        base = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(n_links, fixed_base=False, seed=seed, max_back=max_back, collision_links=(a, b), parallel_axes=axes))
        model = helpers.relaxed_model(base, list(range(16)), mu=0.5)
        assert "P.ct_tree=1" in specialize.spec(model, np.float64, specialize.MODE_STEP_RIGID)
        d = oracle.random_model_data(model, batch_size=6, seed=seed, base_pos_bounds=((-1, -1, 0.0), (1, 1, 0.3)), base_rpy_bounds=((-0.4, -0.4, -3), (0.4, 0.4, 3)))
        truth = helpers.odata_to_block(model, oracle.step(model, d))
        out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
        assert helpers.rel_err(out, truth) < 1e-9, (trial, a, b, axes)
        d32 = helpers.block_to_odata(model, helpers.odata_to_block(model, d).astype(np.float32), d.velocity_representation)
        out32 = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d32))
        e32 = helpers.rel_err(out32, helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32))))
        worst32 = max(worst32, e32)
        assert e32 < 2e-3, (trial, a, b, axes, e32)
    helpers.note("contact_tree_random_trees_fp32_worst", worst32)


@pytest.mark.parametrize("case", ["one_point", "base_link_of_a_fixed_tree", "64_links", "one_link_one_point"])
@pytest.mark.parametrize("kind", ["relaxed", "rigid"])
def test_contact_solve_edge_shapes(reduced_qp, case, kind):
    """[round 5] The edges of the contact problem's shape: a single enabled point (a 3x3 problem, far from a six-lane
    group's width), points only on the base link of a FIXED tree (every column of J is null: the forces are whatever the
    regularisation says and move nothing), a 64-link tree with boxes on its first, middle and last link (one link per
    lane of a full wave), and a single link with a single point."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    if case == "one_point":
        base, idx = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(6, fixed_base=False, seed=5, collision_links=(5,))), [0]
    elif case == "base_link_of_a_fixed_tree":
        base, idx = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(5, fixed_base=True, seed=1, collision_links=(0,), base_offset=(0.0, 0.0, 0.0))), list(range(8))
    elif case == "64_links":
        base, idx = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(64, fixed_base=False, seed=3, max_back=3, collision_links=(0, 31, 63))), list(range(24))
    else:
        base, idx = ja.JaxSimModel.build_from_model_description(robots.box_urdf()), [0]
    if kind == "rigid" and case == "64_links":
        idx = idx[::2]  # (12 points: the 24-point dense QP on a 64-lane group is minutes of emulation)
    model = helpers.relaxed_model(base, idx, mu=0.5) if kind == "relaxed" else helpers.rigid_model(base, idx, K=1e4, D=1e2, build=dict(solver_options={"solver_tol": 1e-6 if case == "64_links" else 1e-9}))
    # (64 links at solver_tol 1e-9: the ORACLE's own KKT factorisation loses positive definiteness on this tree, as the reference's would)
    d = oracle.random_model_data(model, batch_size=6, seed=3, base_pos_bounds=((-1, -1, -0.2), (1, 1, 0.1)), base_rpy_bounds=((-0.4, -0.4, -3), (0.4, 0.4, 3)))
    truth = helpers.odata_to_block(model, oracle.step(model, d))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, truth) < (1e-9 if kind == "relaxed" else 1e-6), (case, kind)


@pytest.mark.parametrize("fixed_base,max_back", [(True, 1), (False, 1), (False, 3)])
def test_maximum_size_models(models, fixed_base, max_back):
    """The largest supported model: 64 links, one per lane of a full wave; a serial chain makes the tree
    63 levels deep (six pointer-jumping rounds, the link-per-lane ABA sweeps)."""
    import jaxsim_amd as ja
    from jaxsim_amd import robots

    model = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(64, fixed_base=fixed_base, seed=3, max_back=max_back))
    assert eb.layout(model).group == 64
    assert int(model.kin_dyn_parameters.tree_depths().max()) == (63 if max_back == 1 else 31)
    d = oracle.random_model_data(model, batch_size=3, seed=1)
    tau, f = helpers.random_inputs(model, 3, 2, np.float64)
    blk, kw = helpers.odata_to_block(model, d), dict(tau=tau.T, link_forces=f.reshape(3, -1).T, force_repr=2)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(eb.run(model, eb.MODE_STEP, blk, **kw), helpers.odata_to_block(model, ref)) < 1e-9
    di = dataclasses_replace_inertial(d)  # the kernel entry points speak the inertial-fixed representation
    vd, sdd = oracle.forward_dynamics_aba(model, di, joint_forces=tau, link_forces=f)
    kwi = dict(tau=tau.T, link_forces=f.reshape(3, -1).T, force_repr=0)
    assert helpers.rel_err(eb.run(model, eb.MODE_FD, blk, **kwi).T, np.concatenate([vd, sdd], -1)) < 1e-9
    acc = np.random.default_rng(4).uniform(-1, 1, size=(3, 6 + model.dofs()))
    fB, tq = oracle.inverse_dynamics(model, dataclasses_replace_inertial(d), joint_accelerations=acc[:, 6:], base_acceleration=acc[:, :6])
    idn = eb.run(model, eb.MODE_ID, blk, in_acc=acc.T).T
    ref_id = np.concatenate([fB if model.floating_base() else np.zeros_like(fB), tq], -1)
    assert float(np.abs(idn - ref_id).max()) / max(1.0, float(np.abs(ref_id).max())) < 1e-9


def dataclasses_replace_inertial(d):
    import dataclasses

    return dataclasses.replace(d, velocity_representation=VelRepr.Inertial)


@pytest.mark.parametrize("name", ["cartpole", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_actuation_limits_and_torque_speed_curve(models, name, dtype):
    """Row B with every branch live: joints beyond their limits (spring + the `jnp.positive` damper quirk,
    api/actuation_model.py:55-66), |sd| in the three regions of the torque-speed curve (:95-126), the clip
    active.  The GPU twin is test_gpu_parity.py::test_actuation_limits_and_torque_speed_curve_gpu."""
    import jaxsim_amd as ja

    model = helpers.actuation_variant(models(name), seed=3)
    N = 10
    d = helpers.actuation_state(models, name, model, N, 21, dtype)
    rng = np.random.default_rng(5)
    tau = rng.uniform(-20, 20, size=(N, model.dofs())).astype(dtype)
    ref = oracle.step(model, helpers.upcast(d), joint_force_references=tau.astype(np.float64))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    plain = helpers.with_params(models(name), actuation_params=ja.ActuationParams())
    off = oracle.step(plain, helpers.upcast(d), joint_force_references=tau.astype(np.float64))
    assert helpers.rel_err(helpers.odata_to_block(model, off), helpers.odata_to_block(model, ref)) > 10 * helpers.tol_of(dtype, name) + 0.02


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 2e-5)])
def test_crba_kernel_matches_oracle(models, name, dtype, tol):
    """MODE_CRBA (composite-rigid-body kernel, rbda/crba.py:10-170): the mass matrix in Mixed representation
    against the oracle's CRBA (body representation) moved to Mixed by the block congruence of
    api/model.py:1529-1590, fixed- and floating-base models."""
    from oracle import refrigid

    model = models(name)
    N = 4
    d = models.random_data(name, N, seed=41, dtype=dtype)
    nv = 6 + model.dofs()
    out = eb.run(model, eb.MODE_CRBA, helpers.odata_to_block(model, d)).T.reshape(N, nv, nv)
    ref = refrigid.free_floating_mass_matrix_mixed(model, helpers.upcast(d))
    scale = max(1.0, np.abs(ref).max())
    assert np.abs(out - ref).max() / scale < tol
    np.testing.assert_array_equal(out, np.transpose(out, (0, 2, 1)))  # mirrored entries are the same numbers


@pytest.mark.parametrize("name", ["cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 2e-5)])
def test_jacobian_kernel_matches_oracle(models, name, dtype, tol):
    """MODE_JAC: doubly-left full Jacobian, its derivative and B_H_L (rbda/jacobian.py:128-339)."""
    from oracle import refrigid

    model = models(name)
    N = 4
    d = models.random_data(name, N, seed=43, dtype=dtype)
    nv, nL = 6 + model.dofs(), model.number_of_links()
    JJ, BH = eb.run(model, eb.MODE_JAC, helpers.odata_to_block(model, d))
    J = JJ[: 6 * nv].T.reshape(N, 6, nv)
    Jd = JJ[6 * nv :].T.reshape(N, 6, nv)
    du = helpers.upcast(d)
    J_ref, BH_ref = refrigid.jacobian_full_doubly_left(model, du.joint_positions)
    Jd_ref = refrigid.jacobian_derivative_full_doubly_left(model, du.joint_positions, du.joint_velocities)
    assert helpers.rel_err(J, J_ref) < tol
    assert helpers.rel_err(Jd, Jd_ref) < tol
    assert helpers.rel_err(BH.T.reshape(N, nL, 3, 4), BH_ref[:, :, :3, :]) < tol


@pytest.mark.parametrize("name", ["cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 3e-4)])
def test_mass_inverse_kernel_matches_oracle(models, name, dtype, tol):
    """MODE_MINV (rbda/mass_inverse.py:11-233): M^-1 in Mixed representation against the inverse of the oracle's
    CRBA matrix.  The reference treats the base of EVERY model as a free 6-DoF body (D0 = I_A[0] is always
    inverted, mass_inverse.py:160-178): for fixed-base models too the result is the inverse of the full (6+n)
    free-floating matrix, and M @ Minv = I."""
    from oracle import refrigid

    model = models(name)
    N = 4
    d = models.random_data(name, N, seed=45, dtype=dtype)
    nv = 6 + model.dofs()
    out = eb.run(model, eb.MODE_MINV, helpers.odata_to_block(model, d)).T.reshape(N, nv, nv).astype(np.float64)
    du = helpers.upcast(d)
    M = refrigid.free_floating_mass_matrix_mixed(model, du)
    ref = np.linalg.inv(M)
    if model.floating_base():
        np.testing.assert_allclose(ref, refrigid.free_floating_mass_matrix_inverse_mixed(model, du), rtol=1e-9, atol=1e-9 * np.abs(ref).max())
    scale = np.abs(ref).max()
    # fp32: the full matrix of a fixed-base model is ill-conditioned (its base block is the composite inertia of
    # the whole tree about a distant point, the inverse has entries of 1e3): ten times the floating-base gate
    assert np.abs(out - ref).max() / scale < (tol if (dtype == np.float64 or model.floating_base()) else 10 * tol)
    if dtype == np.float64:
        np.testing.assert_allclose(M @ out, np.broadcast_to(np.eye(nv), M.shape), atol=1e-8)


# ---- two-wave workgroups (jxs_core.h: run_inertia + run<MODE_STEP, ROLE_MAIN>) ---------------------------
@pytest.mark.parametrize("name", ROW_MODELS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_wave_step_matches_oracle_and_single_wave(models, name, dtype):
    """The two-wave variant of the step kernel (inertia wave, then main wave, on one LDS image): against the
    oracle within the stated tolerance and against the single-wave kernel to rounding (the same arithmetic
    in the same order; only where the bias force meets the rows of Ma differs)."""
    model = models(name)
    if eb.layout(model, dtype).row_mode != 1:
        pytest.skip("model does not use the row-distributed ABA layout")
    N = 6
    d = models.random_data(name, N, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    kw = dict(tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[d.velocity_representation])
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    duo = eb.run(model, eb.MODE_STEP_DUO, helpers.odata_to_block(model, d), **kw)
    solo = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), **kw)
    assert helpers.rel_err(duo, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    assert helpers.rel_err(duo, solo) < (1e-12 if dtype == np.float64 else 2e-5)


def test_two_wave_rollout(models):
    model = models("icub")
    d = models.random_data("icub", 3, seed=12)
    blk = helpers.odata_to_block(model, d)
    out = eb.run(model, eb.MODE_STEP_DUO, blk, n_steps=25)
    for _ in range(25):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8


@pytest.mark.parametrize("name", ["double_pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gravity_torque_kernel_matches_oracle(models, name, dtype):
    """MODE_GRAV (jxs_gravity_torques): the joint part of ``free_floating_gravity_forces`` (api/model.py:1897-1931,
    RNEA at zero velocity and acceleration) from the dedicated kernel -- subtree sums of the link weights."""
    model = models(name)
    N = 5
    d = models.random_data(name, N, seed=21, dtype=dtype)
    ref = oracle.free_floating_gravity_forces(model, helpers.upcast(d))[:, 6:]
    out = eb.run(model, eb.MODE_GRAV, helpers.odata_to_block(model, d)).T[:, 6:]
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(out - ref).max()) / scale < (1e-12 if dtype == np.float64 else 2e-6)


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
@pytest.mark.parametrize("base_velocity", [0.0, 0.3])
def test_fixed_base_rigid_contacts_match_oracle(reduced_qp, kind, base_velocity):
    """[round 3] RigidContacts / RelaxedRigidContacts on a FIXED-base model (a cart on a rail touching the ground).
    The reference solves the contact problem with the inverse of the full free-floating mass matrix -- the base
    answers as a free body -- while the forward dynamics keep it fixed, evaluates J nu and Jdot nu with the stored
    base velocity, and its impact writes a base velocity into the state (rbda/contacts/rigid.py:222-446,
    relaxed_rigid.py:330-420, rbda/mass_inverse.py:118-178): reproduced, checked over several steps so that the
    base velocity written by the first impact feeds the next steps."""
    model, d = pc.fixed_cart_case(kind, 6, base_velocity)
    p, _ = oracle.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    en = np.flatnonzero(model.kin_dyn_parameters.contact_enabled)
    assert (p[:, en, 2] < 0).any() and (p[:, en, 2] > 0).any()
    blk = helpers.odata_to_block(model, d)
    ref = d
    for _ in range(3):
        ref = oracle.step(model, ref)
        blk = eb.run(model, eb.MODE_STEP, blk)
    assert helpers.rel_err(blk, helpers.odata_to_block(model, ref)) < 1e-7
    if kind == "rigid":  # the impact moved the "fixed" base, as in the reference
        assert np.abs(ref.base_linear_velocity).max() > 1e-8


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
@pytest.mark.parametrize("path", ["tree", "dense"])
def test_fifty_point_sphere_matches_oracle(models, reduced_qp, kind, path, monkeypatch):
    """[round 3] More than 32 enabled points (one lane per point, 64-bit point masks): the reference's sphere collision
    shape is 50 points (parsers/rod/utils.py:200-204).  fp64 against the oracle: 1e-7 (RigidContacts: QP + impact) /
    1e-9 (RelaxedRigidContacts).  (The emulation ignores the LDS budget that refuses 50-point RigidContacts in fp64 on
    the device -- two 150 x 150 triangles of doubles are 182 KB; the GPU test runs that case in fp32.)"""
    monkeypatch.setenv("JXS_IGNORE_LDS_BUDGET", "1")
    if path == "dense":  # the default is the solve in the tree (jxs_rigid.inc ta_*); the triangles in the LDS stay covered
        monkeypatch.setenv("JXS_DISABLE_CT_TREE", "1")
    model = pc.sphere50_model(models, kind)
    d = pc.sphere50_data(model, 3)
    p, _ = oracle.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    assert (p[..., 2] < 0).sum(axis=1).min() >= 5
    ref = oracle.step(model, d)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-7 if kind == "rigid" else 1e-9)


# ---- [round 6] system_dynamics / link_contact_forces (SURVEY section 8(a) rows E and I as callable entries) -----------
# reference: src/jaxsim/api/ode.py:16-225, src/jaxsim/api/contact.py:514-603; the kernel modes MODE_DYN / MODE_DYN_RIGID
# (the truth and the error metric: parity_cases.dyn_reference / dyn_err; the blocks here are [rows, N])
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_system_dynamics_matches_oracle(models, name, dtype):
    model = models(name)
    N = 32
    d = models.random_data(name, N, seed=4, dtype=dtype, rep=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, N, 15, dtype)
    ref_blk, ref_W = pc.dyn_reference(model, helpers.upcast(d), tau.astype(np.float64), f.astype(np.float64))
    xdot, W = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=0)
    assert xdot.dtype == dtype
    tol = helpers.tol_of(dtype, name, evaluation=True)
    assert pc.dyn_err(xdot, ref_blk, dtype, env_axis=-1) < tol
    assert pc.dyn_err(W, ref_W.reshape(N, -1).T, dtype, env_axis=-1) < tol
    if name in models.contact_z:
        assert np.abs(ref_W).max() > 1.0  # contacts really act in this sample


def test_system_dynamics_takes_the_torques_as_they_are(models):
    """No actuation model in system_dynamics (api/ode.py:117-122): with limits, friction and a torque-speed curve that all
    bite (helpers.actuation_variant), the joint torques go to ABA unchanged -- while `step` applies the model to them."""
    model = helpers.actuation_variant(models("anymal"), seed=3)
    N = 5
    d = helpers.actuation_state(models, "anymal", model, N, seed=4, dtype=np.float64)
    d = dataclasses.replace(d, velocity_representation=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, N, 5, np.float64)
    ref_blk, _ = pc.dyn_reference(model, d, tau, None)
    xdot, _ = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d), tau=tau.T)
    assert helpers.rel_err(xdot, ref_blk) < 1e-10


@pytest.mark.parametrize("key", ["box4", "anymal16", "anymal4", "chain9f6", "icub8", "planar_biped"])
def test_rigid_system_dynamics_matches_oracle(models, reduced_qp, key):
    model, d = pc.rigid_case(models, key, 8, seed=5)
    d = dataclasses.replace(d, velocity_representation=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref_blk, ref_W = pc.dyn_reference(model, d, tau, f)
    xdot, W = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=0)
    assert helpers.rel_err(xdot, ref_blk) < 1e-6  # (accelerations: the step's 1e-7 gate is on dt x these)
    assert helpers.rel_err(W.T.reshape(8, -1, 6), ref_W) < 1e-6
    assert np.abs(ref_W).max() > 1.0


@pytest.mark.parametrize("key", ["box8", "anymal16", "chain9f6", "icub16", "planar_biped"])
def test_relaxed_system_dynamics_matches_oracle(models, key):
    model, d = pc.relaxed_case(models, key, 8, seed=5)
    d = dataclasses.replace(d, velocity_representation=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, 8, 7, np.float64)
    ref_blk, ref_W = pc.dyn_reference(model, d, tau, f)
    xdot, W = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(8, -1).T, force_repr=0)
    assert helpers.rel_err(xdot, ref_blk) < 1e-8
    assert helpers.rel_err(W.T.reshape(8, -1, 6), ref_W) < 1e-8
    assert np.abs(ref_W).max() > 1.0


# ---- [round 6] height-field terrain (the generic finite-difference normal, terrain.py:40-62) --
def test_height_field_host_class_matches_the_restatement():
    """jaxsim_amd.HeightFieldTerrain (product, host) against oracle.refterrain.GridTerrain (independent statement of the
    bilinear interpolant; normal inherited from the reference's Terrain base class), inside, on and outside the grid; and
    against the sampled function itself at the sample points (exact) and between them (interpolation error only)."""
    t, g, fn = pc.sine_field(extent=1.0, spacing=0.1)
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-1.4, 1.4, 4000), rng.uniform(-1.4, 1.4, 4000)
    np.testing.assert_allclose(t.height(x, y), g.height(x, y), rtol=0, atol=1e-15)
    np.testing.assert_allclose(t.normal(x, y), g.normal(x, y), rtol=0, atol=1e-13)
    xs = -1.0 + 0.1 * np.arange(21)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    np.testing.assert_allclose(t.height(X, Y), fn(X, Y), rtol=0, atol=1e-15)
    inside = (np.abs(x) < 1) & (np.abs(y) < 1)
    assert np.abs(t.height(x[inside], y[inside]) - fn(x[inside], y[inside])).max() < 0.04 * (2.1**2 + 1.7**2) * 0.1**2 / 4  # |f''| h^2 / 8 per axis
    # clamped outside: the border sample extends outwards
    np.testing.assert_allclose(t.height(np.array([5.0]), np.array([0.3])), t.height(np.array([1.0]), np.array([0.3])))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["box", "anymal", "icub"])
def test_height_field_terrain_soft(models, name, dtype):
    t, g, _ = pc.sine_field()
    model = helpers.with_params(models(name), terrain=t)
    N = 12
    d = models.random_data(name, N, seed=23, dtype=dtype)
    ref = oracle.step(helpers.with_params(model, terrain=g), helpers.upcast(d, model))
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    # (fp32: the slope is a difference of two heights 2 cm apart, known to 1e-8 of 0.04 m: 1e-7 in the normal -- nothing)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    flat = eb.run(models(name), eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(flat, helpers.odata_to_block(model, ref)) > 1e-5  # the terrain really changes the answer
    # and the derivative / link wrenches of system_dynamics see the same terrain
    d_in = dataclasses.replace(helpers.upcast(d, model), velocity_representation=VelRepr.Inertial)
    ref_blk, ref_W = pc.dyn_reference(helpers.with_params(model, terrain=g), d_in, None, None)
    xdot, W = eb.run(model, eb.MODE_DYN, helpers.odata_to_block(model, d))
    assert pc.dyn_err(xdot, ref_blk, dtype, env_axis=-1) < max(helpers.tol_of(dtype, name), 1e-3 if dtype == np.float32 else 0)
    assert np.abs(ref_W[..., :2]).max() > 0.1  # tilted normals: horizontal contact forces


@pytest.mark.parametrize("kind,key", [("rigid", "box4"), ("rigid", "anymal4"), ("relaxed", "box8"), ("relaxed", "anymal16")])
def test_height_field_terrain_rigid_models(models, reduced_qp, kind, key):
    t, g, _ = pc.sine_field()
    base, d = pc.contact_case(models, kind, key, 24, seed=5)
    model = helpers.with_params(base, terrain=t)
    ref = oracle.step(helpers.with_params(model, terrain=g), d)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-7 if kind == "rigid" else 1e-9)
    flat = eb.run(base, eb.MODE_STEP, helpers.odata_to_block(model, d))
    assert helpers.rel_err(flat, helpers.odata_to_block(model, ref)) > 1e-5


def test_height_field_known_answer_box_rests_on_a_ramp(models):
    """Known answer without the oracle: a height field that IS a plane (z = tan(a) x) must reproduce PlaneTerrain -- the
    bilinear interpolant of a linear function is that function, its central difference the exact slope."""
    import jaxsim_amd as ja

    a = np.deg2rad(8.0)
    hf = ja.HeightFieldTerrain.from_function(lambda x, y: np.tan(a) * x + 0.0 * y, x_range=(-3, 3), y_range=(-3, 3), spacing=0.25)
    plane = ja.PlaneTerrain.build(height=0.0, normal=[-np.sin(a), 0.0, np.cos(a)])
    box = models("box")
    d = models.random_data("box", 16, seed=3)
    o1 = eb.run(helpers.with_params(box, terrain=hf), eb.MODE_STEP, helpers.odata_to_block(box, d))
    o2 = eb.run(helpers.with_params(box, terrain=plane), eb.MODE_STEP, helpers.odata_to_block(box, d))
    assert helpers.rel_err(o1, o2) < 1e-11


def test_height_field_is_validated(models):
    import jaxsim_amd as ja

    with pytest.raises(ValueError):
        ja.HeightFieldTerrain.build(np.zeros((1, 5)))
    with pytest.raises(ValueError):
        ja.HeightFieldTerrain.build(np.zeros((3, 3)), spacing=(0.1, 0.0))
    with pytest.raises(ValueError):
        ja.HeightFieldTerrain.build(np.full((3, 3), np.nan))


# ---- [round 6] links with more than six children (VERDICT r5 missing 3: kMaxChildren 6 -> 12) --------------------------
@pytest.mark.parametrize("name", ["octopod", "hub12"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_links_with_more_than_six_children(models, name, dtype):
    """An octopod (eight legs on the body: 17 links, 32 lanes) and a twelve-spoke hub (13 links, 16 lanes): every sweep that
    gathers children -- ABA pass 2, RNEA, CRBA, the mass-matrix inverse, gravity torques -- against the oracle."""
    from oracle import refrigid

    model = models(name)
    kdp = model.kin_dyn_parameters
    assert max(np.bincount(np.asarray(kdp.parent_array)[1:])) == (8 if name == "octopod" else 12)
    N = 5
    d = models.random_data(name, N, seed=4, dtype=dtype)
    du = helpers.upcast(d)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    blk = helpers.odata_to_block(model, d)
    t64, f64 = tau.astype(np.float64), f.astype(np.float64)
    # step (SoftContacts)
    ref = oracle.step(model, du, link_forces=f64, joint_force_references=t64)
    out = eb.run(model, eb.MODE_STEP, blk, tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=REPR_CODE[d.velocity_representation])
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    # forward and inverse dynamics, inertial-fixed
    di = dataclasses.replace(du, velocity_representation=VelRepr.Inertial)
    vd, sdd = oracle.forward_dynamics_aba(model, di, joint_forces=t64, link_forces=f64)
    fd = eb.run(model, eb.MODE_FD, blk, tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=0)
    assert helpers.rel_err(fd.T, np.concatenate([vd, sdd], -1)) < (1e-10 if dtype == np.float64 else 2e-4)
    acc = np.random.default_rng(3).uniform(-2, 2, size=(N, 6 + model.dofs())).astype(dtype)
    fB, tq = oracle.inverse_dynamics(model, di, joint_accelerations=acc[:, 6:].astype(np.float64), base_acceleration=acc[:, :6].astype(np.float64), link_forces=f64)
    idn = eb.run(model, eb.MODE_ID, blk, link_forces=f.reshape(N, -1).T, force_repr=0, in_acc=acc.T).T
    ref_id = np.concatenate([fB, tq], -1)
    assert float(np.abs(idn - ref_id).max()) / max(1.0, float(np.abs(ref_id).max())) < (1e-10 if dtype == np.float64 else 2e-5)
    # mass matrix, its inverse, gravity torques
    nv = 6 + model.dofs()
    M = refrigid.free_floating_mass_matrix_mixed(model, du)
    crba = eb.run(model, eb.MODE_CRBA, blk).T.reshape(N, nv, nv)
    assert np.abs(crba - M).max() / max(1.0, np.abs(M).max()) < (1e-11 if dtype == np.float64 else 2e-5)
    minv = eb.run(model, eb.MODE_MINV, blk).T.reshape(N, nv, nv).astype(np.float64)
    Mi = np.linalg.inv(M)
    assert np.abs(minv - Mi).max() / np.abs(Mi).max() < (1e-9 if dtype == np.float64 else 3e-4)
    g_ref = oracle.free_floating_gravity_forces(model, du)[:, 6:]
    g_out = eb.run(model, eb.MODE_GRAV, blk).T[:, 6:]
    assert float(np.abs(g_out - g_ref).max()) / max(1.0, float(np.abs(g_ref).max())) < (1e-12 if dtype == np.float64 else 2e-6)


@pytest.mark.parametrize("kind,idx", [("rigid", OCTOPOD_FEET_4), ("rigid", OCTOPOD_FEET_16), ("relaxed", OCTOPOD_FEET_16)])
def test_octopod_with_the_rigid_contact_models(models, reduced_qp, kind, idx):
    """The contact solves on a hub with eight children: the response sweeps, the (merged) Delassus sweeps and the tree
    solve of RelaxedRigidContacts gather children too (jxs_rigid.inc)."""
    N = 8
    model, d = pc.octopod_case(models, kind, idx, N)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = eb.run(model, eb.MODE_STEP, helpers.odata_to_block(model, d), tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=2)
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-7 if kind == "rigid" else 1e-10)
    if kind == "rigid":
        assert (~reduced_qp.rigid_problem(model, d)["inactive"]).any()
    else:
        from oracle import refrelaxed

        assert refrelaxed.relaxed_problem(model, d)["active"].any()
