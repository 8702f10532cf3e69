"""GPU parity tests (``-m gpu``): the gfx950 kernels, called through the C-ABI via the Python
mirror of the reference API, against the oracle on the same seeded inputs.  Tolerances are
stated in ``helpers.py`` (fp64 1e-10, fp32 1e-3 worst case -- the rigid-contact models keep 3e-3 --, relative to the fp64 oracle)."""

import dataclasses

import numpy as np
import pytest

import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import oracle
import parity_cases as pc
from helpers import REP, to_gpu
from jaxsim_amd import runtime
from oracle import VelRepr
from parity_cases import ALL, OCTOPOD_FEET_4, OCTOPOD_FEET_16, RELAXED_CASES, REPS, RIGID_CASES, reduced_qp  # noqa: F401

pytestmark = pytest.mark.gpu


def test_native_library_is_the_one_in_tree():
    from jaxsim_amd import _lib

    import os

    assert runtime.device_count() >= 1
    assert not os.environ.get("JAXSIM_AMD_LIB")
    assert _lib.LIB_PATH.exists() and "jaxsim_amd/csrc/libjaxsim_amd.so" in str(_lib.LIB_PATH)
    _lib.load()
    # the mapped object must be THE in-tree file (resolved path), not merely something of that name
    mapped = {ln.split()[-1] for ln in open("/proc/self/maps") if "libjaxsim_amd" in ln}
    assert mapped == {str(_lib.LIB_PATH.resolve())}, mapped


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_step_matches_oracle(models, name, dtype):
    model = models(name)
    N = 70  # not a multiple of the environments per wave: exercises the tail masking
    d = models.random_data(name, N, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert out.dtype == dtype
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)


@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed])
def test_step_link_force_representations(models, rep):
    model = models("icub")
    N = 33
    d = models.random_data("icub", N, seed=8, rep=rep)
    tau, f = helpers.random_inputs(model, N, 9, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


def test_step_is_functional_and_inplace_variant_agrees(models):
    model = models("icub")
    d = models.random_data("icub", 16, seed=2, dtype=np.float32)
    g = to_gpu(model, d)
    before = g.state_block()
    out = js.model.step(model, g)
    np.testing.assert_array_equal(g.state_block(), before)  # input untouched
    g2 = to_gpu(model, d)
    out2 = js.model.step(model, g2, inplace=True)
    np.testing.assert_array_equal(out.state_block(), out2.state_block())
    np.testing.assert_array_equal(g2.state_block(), out2.state_block())


@pytest.mark.parametrize("name", ["cartpole", "anymal", "icub"])
def test_rollout_matches_oracle(models, name):
    model = models(name)
    d = models.random_data(name, 8, seed=12)
    out = js.model.rollout(model, to_gpu(model, d), 25)
    for _ in range(25):
        d = oracle.step(model, d)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, d)) < 1e-8


# reference known answer on the GPU: tests/test_simulations.py:194-242
@pytest.mark.parametrize("dtype,atol", [(np.float64, 1e-9), (np.float32, 2e-5)])
def test_box_settles_on_soft_ground_gpu(models, dtype, atol):
    model = models("box")
    params = js.contact.estimate_good_contact_parameters(
        model, number_of_active_collidable_points_steady_state=4, static_friction_coefficient=1.0,
        damping_ratio=1.0, max_penetration=0.001,
    )  # fmt: skip
    model = helpers.enable_points(helpers.with_params(model, contact_params=params), [0, 1, 2, 3])
    data = js.data.JaxSimModelData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=ja.VelRepr.Inertial, dtype=dtype)
    data = js.model.rollout(model, data, 1000)
    p = data.base_position
    np.testing.assert_allclose(p[:2], 0.0, atol=atol)
    np.testing.assert_allclose(p[2] + 0.001, 0.05, rtol=1e-7 if dtype == np.float64 else 1e-4, atol=atol)


@pytest.mark.parametrize("name", ["double_pendulum", "cartpole", "chain5", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Mixed, VelRepr.Body])
def test_forward_dynamics_matches_oracle(models, name, dtype, rep):
    model = models(name)
    N = 21
    d = models.random_data(name, N, seed=6, dtype=dtype, rep=rep)
    tau, f = helpers.random_inputs(model, N, 7, dtype)
    vd, sdd = oracle.forward_dynamics_aba(model, helpers.upcast(d), joint_forces=tau.astype(np.float64), link_forces=f.astype(np.float64))
    gvd, gsdd = js.model.forward_dynamics_aba(model, to_gpu(model, d), joint_forces=tau, link_forces=f)
    tol = helpers.tol_of(dtype, name, evaluation=True)
    assert helpers.rel_err(gsdd, sdd) < tol and helpers.rel_err(gvd, vd) < tol


@pytest.mark.parametrize("name", ["cartpole", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Mixed, VelRepr.Body])
def test_inverse_dynamics_matches_oracle(models, name, dtype, rep):
    model = models(name)
    N = 21
    d = models.random_data(name, N, seed=16, dtype=dtype, rep=rep)
    _, f = helpers.random_inputs(model, N, 17, dtype)
    acc = np.random.default_rng(3).uniform(-2, 2, size=(N, 6 + model.dofs())).astype(dtype)
    a64 = acc.astype(np.float64)
    fB, tau = oracle.inverse_dynamics(model, helpers.upcast(d), joint_accelerations=a64[:, 6:], base_acceleration=a64[:, :6],
                                      link_forces=f.astype(np.float64))  # fmt: skip
    gfB, gtau = js.model.inverse_dynamics(model, to_gpu(model, d), joint_accelerations=acc[:, 6:], base_acceleration=acc[:, :6], link_forces=f)
    ref = np.concatenate([fB if model.floating_base() else np.zeros_like(fB), tau], -1)
    got = np.concatenate([gfB if model.floating_base() else np.zeros_like(gfB), gtau], -1)
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(got - ref).max()) / scale < helpers.tol_of(dtype, name, evaluation=True)


def test_bias_and_gravity_forces(models):
    model = models("anymal")
    d = models.random_data("anymal", 9, seed=21)
    g = to_gpu(model, d)
    assert helpers.rel_err(js.model.free_floating_bias_forces(model, g), oracle.free_floating_bias_forces(model, d)) < 1e-9
    assert helpers.rel_err(js.model.free_floating_gravity_forces(model, g), oracle.free_floating_gravity_forces(model, d)) < 1e-9


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "chain5", "chain9f", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cached_kinematics_match_oracle(models, name, dtype):
    model = models(name)
    d = models.random_data(name, 10, seed=31, dtype=dtype)
    g = to_gpu(model, d)
    t = helpers.upcast(d).update_caches(model)
    assert helpers.rel_err(g._link_transforms, t.link_transforms) < helpers.tol_of(dtype, name, evaluation=True)
    assert helpers.rel_err(g._link_velocities, t.link_velocities) < helpers.tol_of(dtype, name, evaluation=True)


def test_data_build_and_properties(models):
    model = models("icub")
    d = models.random_data("icub", 5, seed=3)
    W_v = d.base_velocity(VelRepr.Mixed)
    g = js.data.JaxSimModelData.build(
        model, base_position=d.base_position, base_quaternion=d.base_quaternion, joint_positions=d.joint_positions,
        base_linear_velocity=W_v[:, :3], base_angular_velocity=W_v[:, 3:], joint_velocities=d.joint_velocities,
        velocity_representation=ja.VelRepr.Mixed,
    )  # fmt: skip
    np.testing.assert_allclose(g._base_linear_velocity, d.base_linear_velocity, atol=1e-12)  # stored inertial-fixed
    np.testing.assert_allclose(g.base_velocity, W_v, atol=1e-12)
    np.testing.assert_allclose(g.generalized_velocity[:, 6:], d.joint_velocities)
    with g.switch_velocity_representation(ja.VelRepr.Body):
        np.testing.assert_allclose(g.base_velocity, d.base_velocity(VelRepr.Body), atol=1e-12)
    r = g.replace(model, base_quaternion=2 * d.base_quaternion)
    np.testing.assert_allclose(r.base_quaternion, d.base_quaternion, atol=1e-12)  # re-normalised (data.py:434-440)
    single = js.data.JaxSimModelData.build(model, base_position=[0, 0, 1.0])
    assert single.base_position.shape == (3,) and single.joint_positions.shape == (23,)
    with pytest.raises(ValueError):
        js.data.JaxSimModelData.build(model, joint_positions=np.zeros(5))


@pytest.mark.parametrize("name", ["icub", "anymal", "cartpole", "double_pendulum"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kernels", ["common_variant", "run_time_flags"])
def test_step_matches_oracle_through_the_librarys_own_kernels(models, name, dtype, kernels, monkeypatch, knobs):
    """[ADVICE r2] The zoo models above have pre-built model-specialised kernels, so every other step test runs those.
    Here the same step goes through what a model WITHOUT a specialised object gets: the ahead-of-time common-feature
    variant (`KV_COMMON`, floating-base soft-contact models in the row layout) and the kernel that reads every flag at
    run time (`KV_GENERIC`)."""
    from jaxsim_amd import runtime, specialize

    model = models(name)
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "0")
    if kernels == "run_time_flags":
        knobs("JXS_DISABLE_COMMON_VARIANT", 1)
    model.__dict__.pop("_device", None)
    try:
        N = 70
        d = models.random_data(name, N, seed=4, dtype=dtype)
        tau, f = helpers.random_inputs(model, N, 5, dtype)
        ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
        out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
        assert specialize.modes(runtime.device_model(model, dtype)) == []
        assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    finally:
        model.__dict__.pop("_device", None)


# ---- BASELINE.json full sizes: size-independent properties ---------------------------------------


def test_full_size_round_trip_fd_id(models):
    """N = 1024, iCub, fp32: RNEA(ABA(tau, f)) = tau and zero base wrench (tests/test_api_model.py:551-577)."""
    model = models("icub")
    N = 1024
    d = models.random_data("icub", N, seed=77, dtype=np.float32, rep=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, N, 78, np.float32)
    g = to_gpu(model, d)
    vd, sdd = js.model.forward_dynamics_aba(model, g, joint_forces=tau, link_forces=f)
    fB, tau_id = js.model.inverse_dynamics(model, g, joint_accelerations=sdd, base_acceleration=vd, link_forces=f)
    scale = float(np.abs(tau).max())
    # ID(FD(tau)) = tau: worst environment within the stated fp32 tolerance, typical far below
    err = np.abs(tau_id - tau).max(axis=1) / scale
    assert err.max() < 2 * helpers.FP32_TOL and np.median(err) < 1e-5
    assert float(np.abs(fB).max()) / max(scale, float(np.abs(f).max())) < 1e-2


def test_full_size_quadruped_step_error_distribution(models):
    """The quadruped at full batch size, fp32: per-environment error distribution against the fp64 oracle on the same
    state, gated at three times what was measured on MI355X (profiles/r04_fp32_error_gpu.txt: median 1.0e-7, 99th
    percentile 1.5e-5 .. 2.0e-5, worst 3.0e-5 .. 3.6e-5 over 2 x 512 states; the reference's own formulation run in
    fp32: 99th percentile 6.9e-5 .. 9.3e-5, worst 2.9e-4 .. 3.7e-4).  [round 4: the round-3 figures, 6e-5 / 3.6e-4,
    were measured against a truth with fp32-rounded kinematics caches -- helpers.upcast.]"""
    model = models("anymal")
    N = 1024
    d = models.random_data("anymal", N, seed=9, dtype=np.float32)
    truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d)))
    out = js.model.step(model, to_gpu(model, d)).state_block()
    per_env = (np.abs(out - truth) / np.maximum(1.0, np.abs(truth))).max(axis=0)
    # worst case: the model's gate -- except for environments on an edge of the discontinuous contact model, which are bound
    # by what the fp64 oracle itself does under one ulp of input noise (helpers.oracle_sensitivity; 2e-4 at seed 9)
    sens = helpers.oracle_sensitivity(model, d)
    bound = np.maximum(helpers.tol_of(np.float32, "anymal"), 10.0 * sens)
    assert (per_env < bound).all(), (per_env.max(), int(np.argmax(per_env / bound)), sens[np.argmax(per_env / bound)])
    assert per_env.max() < helpers.FP32_TOL
    assert np.median(per_env) < 3.6e-7 and np.percentile(per_env, 99) < 6e-5, (np.median(per_env), np.percentile(per_env, 99))


def test_full_size_batch_independence(models):
    """Environments never interact: stepping 1024 envs equals stepping two halves, bitwise."""
    model = models("icub")
    d = models.random_data("icub", 1024, seed=5, dtype=np.float32)
    blk = helpers.odata_to_block(model, d)
    full = js.model.rollout(model, js.data.JaxSimModelData.from_state_block(model, blk), 5).state_block()
    a = js.model.rollout(model, js.data.JaxSimModelData.from_state_block(model, np.ascontiguousarray(blk[:, :512])), 5).state_block()
    b = js.model.rollout(model, js.data.JaxSimModelData.from_state_block(model, np.ascontiguousarray(blk[:, 512:])), 5).state_block()
    np.testing.assert_array_equal(full, np.concatenate([a, b], axis=1))


def test_full_size_step_matches_oracle_and_keeps_unit_quaternion(models):
    model = models("icub")
    N = 1024
    d = models.random_data("icub", N, seed=9, dtype=np.float32)
    ref = oracle.step(model, helpers.upcast(d))
    out = js.model.step(model, to_gpu(model, d))
    truth = helpers.odata_to_block(model, ref)
    assert helpers.rel_err(out.state_block(), truth) < helpers.FP32_TOL
    per_env = (np.abs(out.state_block() - truth) / np.maximum(1.0, np.abs(truth))).max(axis=0)
    # distribution with the anchored ABA (measured on MI355X: median 1.4e-6, p99 1.4e-4)
    assert np.median(per_env) < 3e-6 and np.percentile(per_env, 99) < 3e-4
    # 50 more steps with the estimator's contact parameters (the reference's own recipe; with the
    # default K = 1e6 some of these random deep-penetration states diverge in the oracle as well)
    soft = helpers.with_params(model, contact_params=js.contact.estimate_good_contact_parameters(
        model, number_of_active_collidable_points_steady_state=16, damping_ratio=0.2))
    q = js.model.rollout(soft, to_gpu(soft, d), 50).base_quaternion
    assert np.isfinite(q).all()
    np.testing.assert_allclose(np.linalg.norm(q, axis=-1), 1.0, atol=1e-6)


def test_full_size_airborne_momentum_and_free_fall(models):
    """No contact, no actuation, no joint friction: the CoM follows the free-fall parabola
    and the angular momentum about the CoM is conserved (checked through the oracle's CoM)."""
    model = models("icub")
    N = 1024
    d = oracle.random_model_data(model, batch_size=N, seed=13, dtype=np.float64, base_pos_bounds=((-1, -1, 2.0), (1, 1, 3.0)))
    g = to_gpu(model, d)
    com0 = oracle.com_position(model, d)
    k = 100
    out = js.model.rollout(model, g, k)
    dk = helpers.block_to_odata(model, out.state_block())
    comk = oracle.com_position(model, dk)
    # the CoM velocity at t0 from a one-step finite difference of the oracle-free GPU rollout
    d1 = helpers.block_to_odata(model, js.model.rollout(model, g, 1).state_block())
    v0 = (oracle.com_position(model, d1) - com0) / model.time_step
    t = k * model.time_step
    expected = com0 + v0 * t
    expected[:, 2] += 0.5 * model.gravity * (t * t - t * model.time_step)  # semi-implicit Euler parabola after the 1st step
    np.testing.assert_allclose(comk, expected, atol=2e-4)


def test_device_tables_follow_model_edits(models):
    model = models("cartpole")
    d = models.random_data("cartpole", 4, seed=1)
    g = to_gpu(model, d)
    a = js.model.step(model, g).state_block()
    m2 = helpers.with_params(model, time_step=2e-3)
    b = js.model.step(m2, to_gpu(m2, d)).state_block()
    ref = oracle.step(m2, d)
    assert not np.array_equal(a, b)
    assert helpers.rel_err(b, helpers.odata_to_block(m2, ref)) < helpers.FP64_TOL


@pytest.mark.parametrize("name", ["double_pendulum", "cartpole", "box", "chain9f", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_golden(models, name, dtype):
    """The committed golden fixtures (tests/golden, oracle-generated) through the C-ABI."""
    import pathlib

    g = dict(np.load(pathlib.Path(__file__).resolve().parent / "golden" / f"{name}.npz"))
    model = models(name)
    data = js.data.JaxSimModelData.from_state_block(model, g["state"].astype(dtype), ja.VelRepr.Inertial)
    out = js.model.step(model, data, link_forces=g["link_forces"], joint_force_references=g["tau"])
    assert helpers.rel_err(out.state_block(), g["step"]) < helpers.tol_of(dtype, name)
    vd, sdd = js.model.forward_dynamics_aba(model, data, joint_forces=g["tau"], link_forces=g["link_forces"])
    assert helpers.rel_err(np.concatenate([vd, sdd], -1), g["fd"]) < helpers.tol_of(dtype, name, evaluation=True)
    assert helpers.rel_err(data._link_transforms, g["link_transforms"]) < helpers.tol_of(dtype, name, evaluation=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_plane_terrain_gpu(models, dtype):
    terrain = ja.PlaneTerrain.build(height=0.02, normal=[0.15, -0.1, 1.0])
    model = helpers.with_params(models("icub"), terrain=terrain)
    d = models.random_data("icub", 40, seed=23, dtype=dtype)
    ref = oracle.step(model, helpers.upcast(d))
    out = js.model.step(model, to_gpu(model, d))
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype)


def test_fused_rollout_equals_repeated_steps_gpu(models, knobs):
    model = models("icub")
    d = models.random_data("icub", 64, seed=14, dtype=np.float32)
    g = to_gpu(model, d)
    fused = js.model.rollout(model, g, 9).state_block()
    # bitwise against the single-wave step kernel (the fused rollout is its loop)
    knobs("JXS_DUO", 0)
    g1 = g
    for _ in range(9):
        g1 = js.model.step(model, g1)
    np.testing.assert_array_equal(fused, g1.state_block())
    # the opt-in two-wave variant forms the bias force from the handed-over rows of Ma in another order: rounding only
    knobs("JXS_DUO", 1)
    for _ in range(9):
        g = js.model.step(model, g)
    assert helpers.rel_err(fused, g.state_block()) < 2e-3  # nine steps of a contact-rich fp32 trajectory
    # more collidable points than lanes (sphere: 50 points, 2 chunks): rollout falls back to launches
    sph = models("sphere")
    ds = models.random_data("sphere", 16, seed=3)
    gs = to_gpu(sph, ds)
    fused = js.model.rollout(sph, gs, 5).state_block()
    for _ in range(5):
        ds = oracle.step(sph, ds)
    assert helpers.rel_err(fused, helpers.odata_to_block(sph, ds)) < 1e-9


@pytest.mark.parametrize("name", ["anymal", "icub", "icub16"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_wave_step_matches_oracle_and_single_wave_gpu(models, name, dtype, knobs, kernel_policy):
    """The opt-in two-wave workgroup variant of the step kernel (JXS_DUO=1; jxs_core.h run_inertia + run<MODE_STEP,
    ROLE_MAIN>): against the oracle within the stated tolerance, against the single-wave kernel to rounding, for a
    ragged batch (an odd number of tiles: the second pair of the last workgroup is empty)."""
    model = models(name)
    N = 2 * 37 + 1
    d = models.random_data(name, N, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    knobs("JXS_DUO", 0)
    solo = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau).state_block()
    knobs("JXS_DUO", 1)
    duo = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau).state_block()
    assert helpers.rel_err(duo, helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    # (fp32: other contraction choices in two instruction streams; measured 4e-5 on the humanoid's contact-rich states)
    assert helpers.rel_err(duo, solo) < (1e-12 if dtype == np.float64 else 1e-4)
    # (fp64: two pairs of waves exceed the 160 KB of LDS of a CU, the single-wave kernel runs; [round 4] the variant is
    # compiled into the library only, -DJXS_WITH_DUO: a model-specialised object ignores the knob)
    if dtype == np.float32 and kernel_policy == "library":
        assert not np.array_equal(duo, solo), "the two-wave variant did not run"


# ---- Runge-Kutta 4 (api/integrators.py:91-167; the softer ground: pc.rk4) --------------------------------------------------
@pytest.mark.parametrize("name", ["box", "sphere", "cartpole", "chain9f", "anymal", "icub16", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rk4_step_matches_oracle_gpu(models, name, dtype):
    model = pc.rk4(models(name))
    N = 70
    d = models.random_data(name, N, seed=31, dtype=dtype)
    tau, f = helpers.random_inputs(model, N, 32, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)


@pytest.mark.parametrize("name,kind", [("icub", "euler"), ("cartpole", "euler"), ("chain9f", "rk4"), ("anymal", "rigid"), ("icub80", "euler")])
def test_controlled_rollout_equals_the_step_loop_gpu(models, name, kind):
    """[round 4] js.model.rollout with a torque SEQUENCE [K, N, n] (jxs_rollout_controlled; jax.lax.scan over step
    with precomputed joint_force_references in the reference): one fused launch with a torque load per step where the
    steps fuse, one launch per step with the step's rows gathered by a strided device copy otherwise (RungeKutta4,
    RigidContacts, several point chunks).  Against the oracle stepping with tau[k]; equal to K single steps on the
    device; not the rollout that holds tau[0]."""
    K, N = 6, 37
    model, d = pc.rollout_case(models, name, kind, N, seed=21)
    n = model.dofs()
    tau = np.random.default_rng(11).uniform(-3, 3, size=(K, N, n))
    ref = d
    for k in range(K):
        ref = oracle.step(model, ref, joint_force_references=tau[k])
    out = js.model.rollout(model, to_gpu(model, d), K, joint_force_references=tau).state_block()
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < (1e-5 if kind == "rigid" else 1e-9)
    data = to_gpu(model, d)
    for k in range(K):
        data = js.model.step(model, data, joint_force_references=tau[k])
    assert helpers.rel_err(out, data.state_block()) < (1e-6 if kind == "rigid" else 1e-11)
    held = js.model.rollout(model, to_gpu(model, d), K, joint_force_references=tau[0]).state_block()
    assert helpers.rel_err(held, out) > 1e-6
    # fp32, fused: same steps as the single launches
    if kind == "euler":
        d32 = helpers.block_to_odata(model, helpers.odata_to_block(model, d).astype(np.float32), d.velocity_representation)
        o32 = js.model.rollout(model, to_gpu(model, d32), K, joint_force_references=tau).state_block()
        s32 = to_gpu(model, d32)
        for k in range(K):
            s32 = js.model.step(model, s32, joint_force_references=tau[k])
        assert o32.dtype == np.float32 and helpers.rel_err(o32, s32.state_block()) < 2e-4


@pytest.mark.parametrize("name,kind,seq", [("icub", "euler", True), ("cartpole", "euler", False), ("chain9f", "rk4", True), ("anymal", "rigid", False), ("icub80", "euler", True), ("icub16", "disabled", True)])
def test_recorded_rollout_returns_every_step_gpu(models, name, kind, seq):
    """[round 4] js.model.rollout(..., return_trajectory=True) / jxs_rollout_recorded: the state after every step (the
    stacked outputs of the reference's jax.lax.scan over step), stored from registers inside the fused launch or copied
    per step where the steps do not fuse.  Every recorded state against the oracle; the last one is the final state;
    recording does not change the rollout (bitwise)."""
    K, N = 5, 37
    model, d = pc.rollout_case(models, name, kind, N, seed=23)
    n = model.dofs()
    tau = np.random.default_rng(13).uniform(-3, 3, size=(K, N, n))
    if not seq:
        tau[:] = tau[0]
    arg = tau if seq else tau[0]
    final, states = js.model.rollout(model, to_gpu(model, d), K, joint_force_references=arg, return_trajectory=True)
    assert states.shape == (K,) + final.state_block().shape
    ref, tol = d, (1e-5 if kind == "rigid" else 1e-9)
    for k in range(K):
        ref = oracle.step(model, ref, joint_force_references=tau[k])
        assert helpers.rel_err(states[k], helpers.odata_to_block(model, ref)) < tol, k
    np.testing.assert_array_equal(states[-1], final.state_block())
    plain = js.model.rollout(model, to_gpu(model, d), K, joint_force_references=arg).state_block()
    np.testing.assert_array_equal(plain, final.state_block())


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-4)])
def test_rk4_with_more_points_than_lanes_gpu(models, dtype, tol):
    """[round 4] RungeKutta4 + SoftContacts with 80 collidable points on 32 lanes: three chunks, the stage data of the
    chunks behind the first in the LDS (jxs_core.h contact_chunk); one step against the oracle, then ten in place
    (the deformation rows are read at every stage and written at the last) -- was refused up to round 3."""
    model = pc.rk4(pc.icub80())
    N = 37
    d = pc.icub80_data(model, N, dtype)
    rng = np.random.default_rng(5)
    d.tangential_deformation[:] = (1e-3 * rng.normal(size=d.tangential_deformation.shape)).astype(dtype)
    tau, f = helpers.random_inputs(model, N, 7, dtype)
    kw = dict(link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    ref = oracle.step(model, helpers.upcast(d), **kw)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < tol
    if dtype == np.float64:
        ref10 = d
        for _ in range(10):
            ref10 = oracle.step(model, ref10)
        out10 = js.model.rollout(model, to_gpu(model, d), 10).state_block()
        assert helpers.rel_err(out10, helpers.odata_to_block(model, ref10)) < 1e-8


@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed])
def test_rk4_link_force_representations_gpu(models, rep):
    model = pc.rk4(models("icub"))
    d = models.random_data("icub", 33, seed=33, rep=rep)
    tau, f = helpers.random_inputs(model, 33, 34, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


def test_rk4_rollout_and_free_fall_gpu(models):
    model = pc.rk4(models("icub"))
    d = models.random_data("icub", 20, seed=35)
    out = js.model.rollout(model, to_gpu(model, d), 10).state_block()
    for _ in range(10):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8
    # constant acceleration is integrated exactly by RK4
    box = pc.rk4(models("box"))
    v0 = np.array([0.3, -0.2, 1.0])
    d0 = oracle.OracleData.build(box, base_position=[0.0, 0.0, 5.0], base_linear_velocity=v0)
    blk = js.model.rollout(box, to_gpu(box, d0), 50).state_block()
    t = 50 * box.time_step
    expect = np.array([0.0, 0.0, 5.0]) + v0 * t + 0.5 * np.array([0.0, 0.0, box.gravity]) * t * t
    np.testing.assert_allclose(blk[0:3, 0], expect, rtol=0, atol=1e-12)


# ---- RigidContacts (the cases: parity_cases.RIGID_CASES) ----------------------
@pytest.mark.parametrize("key", list(RIGID_CASES))
def test_rigid_step_matches_oracle_gpu(models, reduced_qp, key):
    N = 21  # not a multiple of the environments per wave
    model, d = pc.rigid_case(models, key, N, seed=5)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    # 1e-7: with several points on one rigid body the QP Hessian is singular up to the 1e-6 shift
    # (condition ~1e7), rounding differences between the two implementations are amplified by it
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < 1e-7


# fp32 gates of the rigid-contact steps, PER CASE [round 3]: measured on MI355X (gpurun_out/r03_b/errors.log, the
# values in the comments) x 3, rounded up -- instead of a blanket 3e-3.  The box cases stay near 3e-3: 1 kg,
# K = 1e5 with centimetres of penetration, contact forces of 1e3 N on four coplanar points whose 12x12 Delassus
# matrix has rank 6 plus the 1e-6 shift.
# anymal4 (one point per foot, the merged-sweep models): since the impact reuses the Delassus matrix of the force
# solve as its preconditioner (jxs_rigid.inc rigid_impact) the conjugate gradients stop at their fp32 tolerance
# (3e-5 of the initial residual) instead of landing on the solution in one step: 1.7e-5 where the rebuilt
# preconditioner gave 9.6e-7 (fp64: 1e-9 either way).
RIGID_FP32_TOL = {"anymal4": 5e-5, "icub8": 1.1e-4, "anymal16": 4.5e-5, "box4": 3e-3}  # 1.7e-5, 3.5e-5, 1.4e-5, 1.04e-3
RIGID_RK4_FP32_TOL = {"box4": 2.5e-3, "anymal4": 5e-5, "icub8": 1.8e-4}  # 7.8e-4, < 3e-5, 5.7e-5
RK4FAST_FP32_TOL = {("relaxed", "box8"): 4.5e-5, ("relaxed", "anymal16"): 1.5e-5, ("relaxed", "icub16"): 9e-5, ("rigid", "box4"): 2.5e-3,
                    ("rigid", "anymal4"): 1.1e-4}  # 1.4e-5, 4.6e-6, 2.9e-5, 8.2e-4, 3.5e-5  # fmt: skip


@pytest.mark.parametrize("key,tol", list(RIGID_FP32_TOL.items()))
def test_rigid_step_fp32_gpu(models, reduced_qp, key, tol):
    """fp32 against the fp64 oracle on the same inputs: 3e-3 like the soft-contact path (measured
    3e-6 .. 6e-5 on the articulated models, 1e-3 on the box: 1 kg, K = 1e5 with centimetres of
    penetration, i.e. contact forces of 1e3 N on four coplanar points whose 12x12 Delassus matrix has
    rank 6 plus the 1e-6 shift)."""
    model, d = pc.rigid_case(models, key, 40, seed=5, dtype=np.float32)
    ref = oracle.step(model, helpers.upcast(d))
    out = js.model.step(model, to_gpu(model, d))
    blk = out.state_block()
    assert blk.dtype == np.float32 and np.isfinite(blk).all()
    err = helpers.rel_err(blk, helpers.odata_to_block(model, ref))
    helpers.note(f"rigid_fp32/{key}", err)
    assert err < tol


@pytest.mark.parametrize("dtype,atol", [(np.float64, 1e-4), (np.float32, 2e-4)])
def test_rigid_box_settles_known_answer_gpu(models, dtype, atol):
    """reference tests/test_simulations.py:245-292."""
    model = pc.settling_box(models, "rigid")
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial, dtype=dtype)
    out = js.model.rollout(model, to_gpu(model, d), 1000).state_block()
    assert abs(out[0, 0]) < 1e-6 and abs(out[1, 0]) < 1e-6
    assert out[2, 0] == pytest.approx(0.05, abs=atol)


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
def test_rigid_models_carry_the_tangential_rows_through(models, kind):
    """RigidContacts / RelaxedRigidContacts have no tangential deformation (rigid.py:448-458,
    relaxed_rigid.py:251-263): the rows of the state block are passengers, also out of place and with
    every point enabled."""
    make = helpers.rigid_model if kind == "rigid" else helpers.relaxed_model
    model = make(models("box"), list(range(8)))
    d = models.random_data("box", 9, seed=3)
    assert np.abs(d.tangential_deformation).max() > 0
    out = js.model.step(model, to_gpu(model, d))
    np.testing.assert_array_equal(out.state_block()[13:], helpers.odata_to_block(model, d)[13:])


@pytest.mark.parametrize("key", ["box4", "anymal4", "icub8"])
def test_rigid_rk4_step_matches_oracle_gpu(models, reduced_qp, key):
    """RungeKutta4 with RigidContacts: QP forces at each stage, impact on the integrated state; the
    reference runs its rigid-contact test for every integrator (tests/test_simulations.py:245)."""
    N = 21
    model, d = pc.rigid_case(models, key, N, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < 1e-7
    _, d32 = pc.rigid_case(models, key, N, seed=5, dtype=np.float32)
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    ref32 = oracle.step(model, helpers.upcast(d32))
    err32 = helpers.rel_err(out32, helpers.odata_to_block(model, ref32))
    helpers.note(f"rigid_rk4_fp32/{key}", err32)
    assert out32.dtype == np.float32 and err32 < RIGID_RK4_FP32_TOL[key]


@pytest.mark.parametrize("dtype,atol", [(np.float64, 1e-4), (np.float32, 2e-4)])
def test_rigid_rk4_box_settles_known_answer_gpu(models, dtype, atol):
    """reference tests/test_simulations.py:245-292 with integrator = RungeKutta4."""
    model = pc.settling_box(models, "rigid", ja.IntegratorType.RungeKutta4)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial, dtype=dtype)
    out = js.model.rollout(model, to_gpu(model, d), 1000).state_block()
    assert abs(out[0, 0]) < 1e-6 and abs(out[1, 0]) < 1e-6
    assert out[2, 0] == pytest.approx(0.05, abs=atol)


@pytest.mark.parametrize("kind,key", [("relaxed", "box8"), ("relaxed", "anymal16"), ("relaxed", "icub16"), ("rigid", "box4"), ("rigid", "anymal4")])
def test_rk4fast_step_matches_oracle_gpu(models, reduced_qp, kind, key):
    """RungeKutta4Fast (api/integrators.py:170-276) with the contact models without contact state,
    against oracle/refstep.py::rk4fast_integration (the reference's function as written)."""
    N = 21
    model, d = pc.contact_case(models, kind, key, N, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4Fast)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < (1e-10 if kind == "relaxed" else 1e-7)
    _, d32 = pc.contact_case(models, kind, key, N, seed=5, dtype=np.float32)
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    ref32 = oracle.step(model, helpers.upcast(d32))
    err32 = helpers.rel_err(out32, helpers.odata_to_block(model, ref32))
    helpers.note(f"rk4fast_fp32/{kind}/{key}", err32)
    assert out32.dtype == np.float32 and err32 < RK4FAST_FP32_TOL[(kind, key)]


@pytest.mark.parametrize("kind,key", [("rigid", "anymal16"), ("relaxed", "icub16")])
def test_mfma_cholesky_equals_the_vector_path_bitwise_gpu(models, kind, key, monkeypatch, knobs):
    """[round 3] The blocked Cholesky of the contact solvers with its trailing updates on the matrix cores
    (v_mfma_f32_16x16x4_f32 accumulator tiles, jxs_lanes_device.h ChTiles) -- an opt-in build (-DJXS_MFMA_CHOLESKY,
    measured slower end to end, profiles/r03_mfma_cholesky_experiment.md), here as a model-specialised kernel built
    with that flag.  It performs the same fused multiply-adds in the same order as the vector path: the fp32 step
    results must be IDENTICAL to those of its own vector path (JXS_NO_MFMA=1; and equal to the default build's up to the
    rounding of another compilation), over several steps of
    random states and of standing ones (every sole point active)."""
    from jaxsim_amd import runtime, specialize

    model, d_random = pc.contact_case(models, kind, key, 37, seed=5, dtype=np.float32)

    def run(d):
        g = to_gpu(model, d)
        for _ in range(3):
            g = js.model.step(model, g)
        return g.state_block()

    datas = (d_random, helpers.standing_data(model, 37, seed=2, dtype=np.float32, noise=0.003))
    model.__dict__.pop("_device", None)
    default = [run(d) for d in datas]
    monkeypatch.setenv("JAXSIM_AMD_SPEC_EXTRA_FLAGS", "-DJXS_MFMA_CHOLESKY")
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "1")  # (pre-built by __graft_entry__.build(); built here otherwise)
    model.__dict__.pop("_device", None)
    try:
        assert specialize.modes(runtime.device_model(model, np.float32)) == [specialize.MODE_STEP_RIGID]
        tiles = [run(d) for d in datas]
        knobs("JXS_NO_MFMA", 1)
        vector = [run(d) for d in datas]
    finally:
        model.__dict__.pop("_device", None)
    for a, b, c in zip(default, tiles, vector):
        assert np.isfinite(b).all()
        np.testing.assert_array_equal(b, c)  # the two paths of ONE binary: bit for bit
        # the default library is another compilation (other contraction choices outside the factorisation): rounding
        assert helpers.rel_err(b, a) < 1e-4


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
@pytest.mark.parametrize("base_velocity", [0.0, 0.3])
def test_fixed_base_rigid_contacts_match_oracle_gpu(reduced_qp, kind, base_velocity):
    """[round 3] RigidContacts / RelaxedRigidContacts on a FIXED-base model (a cart on a rail touching the ground):
    the contact solve with the base as a free body (the reference inverts the full free-floating mass matrix for every
    model), fixed-base forward dynamics, J nu / Jdot nu with the stored base velocity, and an impact that writes a
    base velocity into the state -- as rbda/contacts/rigid.py:222-446 and relaxed_rigid.py:330-420 do.  Three steps,
    fp64 1e-7 against the oracle; fp32 within 1e-3."""
    model, d = pc.fixed_cart_case(kind, 41, base_velocity)
    ref, g = d, to_gpu(model, d)
    for _ in range(3):
        ref = oracle.step(model, ref)
        g = js.model.step(model, g)
    assert helpers.rel_err(g.state_block(), helpers.odata_to_block(model, ref)) < 1e-7
    if kind == "rigid":
        assert np.abs(ref.base_linear_velocity).max() > 1e-8  # the impact moved the "fixed" base, as in the reference
    _, d32 = pc.fixed_cart_case(kind, 41, base_velocity, dtype=np.float32)
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    err32 = helpers.rel_err(out32, helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32))))
    helpers.note(f"fixed_base_fp32/{kind}/{base_velocity}", err32)
    assert out32.dtype == np.float32 and err32 < 1e-3


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
def test_fifty_point_sphere_matches_oracle_gpu(models, reduced_qp, kind):
    """More than 32 enabled points with the rigid contact models: the reference's 50-point sphere collision shape
    (parsers/rod/utils.py:200-204), one lane per point in a 64-lane group.  RelaxedRigidContacts in fp64 (1e-9) and fp32.
    [round 4] RigidContacts in fp64 too (1e-7): round 3 refused it -- two 150 x 150 triangles of doubles, 182 KB, exceed
    the LDS of a CU -- the solve in the tree (jxs_rigid.inc ta_*) needs no triangle."""
    model = pc.sphere50_model(models, kind)
    d = pc.sphere50_data(model, 9)
    out = js.model.step(model, to_gpu(model, d))
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, oracle.step(model, d))) < (1e-9 if kind == "relaxed" else 1e-7)
    d32 = pc.sphere50_data(model, 9, np.float32)
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    err32 = helpers.rel_err(out32, helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32))))
    helpers.note(f"sphere50_fp32/{kind}", err32)
    assert out32.dtype == np.float32 and np.isfinite(out32).all() and err32 < 3e-3


def test_rk4fast_is_refused_for_soft_contacts_gpu(models):
    with pytest.raises(Exception, match="RungeKutta4Fast"):
        model = helpers.with_params(models("box"), integrator=ja.IntegratorType.RungeKutta4Fast)
        js.model.step(model, to_gpu(model, models.random_data("box", 2)))


@pytest.mark.parametrize("kind", ["rigid", "relaxed"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_contact_solves_do_not_depend_on_wave_mates(models, kind, dtype):
    """Several environments share a wave (4 for the quadruped) and its wave-uniform decisions (which
    block columns to skip, when to stop refining / iterating): an environment stepped alone gives the
    bits it gives inside a batch, like under the reference's vmap."""
    make = helpers.rigid_model if kind == "rigid" else helpers.relaxed_model
    params = dict(K=1e4, D=1e2) if kind == "rigid" else dict(mu=0.5)
    model = make(models("anymal"), helpers.ANYMAL_FEET_16, **params)
    d = models.random_data("anymal", 13, seed=5, dtype=dtype)
    blk = helpers.odata_to_block(model, d)
    full = js.model.step(model, to_gpu(model, d)).state_block()
    for e in (0, 1, 6, 12):
        one = js.data.JaxSimModelData.from_state_block(model, blk[:, [e]], ja.VelRepr.Mixed)
        np.testing.assert_array_equal(js.model.step(model, one).state_block()[:, 0], full[:, e])


def test_rigid_tumbling_box_rollout_gpu(models, reduced_qp):
    model, d = pc.tumbling_box(models, "rigid")
    out = js.model.rollout(model, to_gpu(model, d), 300).state_block()
    for _ in range(300):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-7


def test_config5_quadruped_rigid_contacts_with_gravity_compensation(models, reduced_qp):
    """BASELINE.json config 5: quadruped, RigidContacts, tau = RNEA gravity term, fp32, batch 4096.
    Oracle parity on a slice of the batch (fp64 truth), device-resident controller loop, finiteness
    and batch independence at the full size."""
    model = helpers.rigid_model(models("anymal"), helpers.ANYMAL_FEET_4, K=1e4, D=2e2)
    N = 4096
    d32 = models.random_data("anymal", N, seed=11, dtype=np.float32)
    g = to_gpu(model, d32)
    tau = js.model.gravity_compensation_torques(model, g)
    runtime.synchronize()
    # the device torque block equals the joint part of free_floating_gravity_forces
    gq = js.model.free_floating_gravity_forces(model, g)[:, 6:]
    np.testing.assert_allclose(tau.to_host().T, gq, rtol=1e-5, atol=1e-4)
    sub = dataclasses.replace(helpers.upcast(d32), **{
        f.name: getattr(helpers.upcast(d32), f.name)[:24] for f in dataclasses.fields(d32)
        if isinstance(getattr(d32, f.name), np.ndarray)})  # fmt: skip
    ref_tau = oracle.free_floating_gravity_forces(model, sub)[:, 6:]
    np.testing.assert_allclose(gq[:24], ref_tau, rtol=1e-4, atol=1e-3)
    out = js.model.step(model, g, joint_force_references=tau).state_block()
    assert np.isfinite(out).all()
    ref = oracle.step(model, sub, joint_force_references=ref_tau)
    assert helpers.rel_err(out[:, :24], helpers.odata_to_block(model, ref)) < 3e-3
    # batch independence: the first 24 environments alone give the same bits
    g24 = js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d32)[:, :24], ja.VelRepr.Mixed)
    out24 = js.model.step(model, g24, joint_force_references=tau.to_host()[:, :24].T).state_block()
    np.testing.assert_array_equal(out24, out[:, :24])


@pytest.mark.parametrize("n_links,seed,max_back,links,axes", [(7, 31, 1, (0, 6), None), (12, 32, 3, (0, 11), None), (20, 33, 2, (3, 19), None), (14, 34, 1, (2, 11), "all"),
                                                              (16, 100, 3, (9, 11), None), (12, 35, 1, (0, 11), "all"), (18, 36, 2, (1, 4, 9, 17), "aligned")])  # fmt: skip
@pytest.mark.parametrize("kind", ["relaxed", "rigid"])
def test_contact_tree_solve_on_random_trees_gpu(reduced_qp, kind, n_links, seed, max_back, links, axes, monkeypatch):
    """[round 5] The contact solve in the tree (jxs_rigid.inc ta_*) on random floating trees -- serial and branching, 7 to
    20 links, mixed revolute / prismatic joints, and [VERDICT r4 weak #1] trees whose joint axes are all parallel or
    axis-aligned -- with the contact boxes on the given links (two links, neighbours or far apart; four links):
    RelaxedRigidContacts and RigidContacts in fp64 against the oracle, and RelaxedRigidContacts in fp32.  Every case takes
    the tree (round 4's link space took pairs six or more joints apart only, and was wrong for the parallel-axis ones)."""
    from jaxsim_amd import robots, specialize

    base = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(n_links, fixed_base=False, seed=seed, max_back=max_back, collision_links=links, parallel_axes=axes))
    idx = list(range(8 * len(links)))
    # [ADVICE r5] RigidContacts at solver_tol = 1e-7: at the default 1e-3 the tree's and the oracle's iterates agree only to the
    # accuracy at which the iteration stops (the gate had to be 1e-5); at 1e-7 both are converged and the gate is tight again
    model = (helpers.relaxed_model(base, idx, mu=0.5) if kind == "relaxed"
             else helpers.rigid_model(base, idx, build=dict(solver_options={"solver_tol": 1e-7}), K=1e4, D=1e2))
    if kind == "rigid":  # (RigidContacts takes the tree by default only where the triangles do not fit the LDS: the knob runs it here)
        assert "P.ct_tree=0" in specialize.spec(model, np.float64, specialize.MODE_STEP_RIGID)
        monkeypatch.setenv("JXS_CT_TREE_RIGID", "1")
    assert "P.ct_tree=1" in specialize.spec(model, np.float64, specialize.MODE_STEP_RIGID)
    N = 9
    d = oracle.random_model_data(model, batch_size=N, seed=seed, base_pos_bounds=((-1, -1, 0.0), (1, 1, 0.25)), base_rpy_bounds=((-0.4, -0.4, -3), (0.4, 0.4, 3)))
    ref = helpers.odata_to_block(model, oracle.step(model, d))
    out = js.model.step(model, to_gpu(model, d)).state_block()
    err = helpers.rel_err(out, ref)
    helpers.note(f"contact_tree_random_fp64/{kind}/{n_links}", err)
    assert err < (1e-9 if kind == "relaxed" else 1e-6)
    assert js.model.solver_fault_counts(model, np.float64) == (0, 0)
    if kind == "relaxed":
        d32 = oracle.random_model_data(model, batch_size=N, seed=seed, dtype=np.float32, base_pos_bounds=((-1, -1, 0.0), (1, 1, 0.25)),
                                       base_rpy_bounds=((-0.4, -0.4, -3), (0.4, 0.4, 3)))  # fmt: skip
        out32 = js.model.step(model, to_gpu(model, d32)).state_block()
        err32 = helpers.rel_err(out32, helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32))))
        helpers.note(f"contact_tree_random_fp32/{n_links}", err32)
        assert err32 < 3e-3


def test_queries_of_a_model_without_joints_gpu(models):
    """[round 5] A single floating link (n = 0): every query takes the EMPTY joint arrays the reference takes
    (`inverse_dynamics(joint_accelerations=jnp.zeros(0))`) -- found by tools/fuzz/gpu_campaign_queries.py, whose one-link
    trees raised a ValueError in the host wrapper of `inverse_dynamics` (reshape(-1, 0))."""
    model = models("box")
    N = 5
    d = models.random_data("box", N, seed=3)
    g = to_gpu(model, d)
    _, f = helpers.random_inputs(model, N, 4, np.float64)
    acc = np.random.default_rng(5).uniform(-2, 2, size=(N, 6))
    for ja_ in (np.zeros((N, 0)), np.zeros(0), None):
        fB, tau = js.model.inverse_dynamics(model, g, joint_accelerations=ja_, base_acceleration=acc, link_forces=f)
        rB, rtau = oracle.inverse_dynamics(model, d, joint_accelerations=np.zeros((N, 0)), base_acceleration=acc, link_forces=f)
        assert tau.shape == (N, 0) and helpers.rel_err(fB, rB) < 1e-10
    vd, sdd = js.model.forward_dynamics_aba(model, g, joint_forces=np.zeros((N, 0)), link_forces=f)
    rvd, _ = oracle.forward_dynamics_aba(model, d, joint_forces=np.zeros((N, 0)), link_forces=f)
    assert sdd.shape == (N, 0) and helpers.rel_err(vd, rvd) < 1e-10
    assert helpers.rel_err(js.model.free_floating_mass_matrix(model, g), oracle.free_floating_mass_matrix(model, d)) < 1e-12
    assert helpers.rel_err(js.model.free_floating_bias_forces(model, g), oracle.free_floating_bias_forces(model, d)) < 1e-10
    assert helpers.rel_err(js.model.free_floating_gravity_forces(model, g), oracle.free_floating_gravity_forces(model, d)) < 1e-10
    assert helpers.rel_err(js.model.free_floating_mass_matrix_inverse(model, g) @ oracle.free_floating_mass_matrix(model, d), np.broadcast_to(np.eye(6), (N, 6, 6))) < 1e-9
    J, Jd, _ = js.model.jacobian_full_doubly_left(model, g)
    assert J.shape[-1] == 6 and Jd.shape[-1] == 6
    out = js.model.rollout(model, g, 3, joint_force_references=np.zeros((3, N, 0))).state_block()
    dk = d
    for _ in range(3):
        dk = oracle.step(model, dk)
    assert helpers.rel_err(out, helpers.odata_to_block(model, dk)) < 1e-9


def test_fuzz_campaign_slice_on_the_device(tmp_path):
    """[round 5] A slice of tools/fuzz/gpu_campaign.py: 60 random trees (1 to 40 links, SoftContacts / RelaxedRigidContacts
    -- one chunk and chunked -- / RigidContacts, semi-implicit Euler / RungeKutta4, fp64 and fp32) prepared on the host
    (oracle truth, the emulation's result, the fp32 sensitivities), then stepped through the product on the device: fp64
    within the class tolerances of the truth and 1e-9 of the emulation, fp32 within what the case's own measured
    sensitivity allows.  The full campaign (1500 trees, 2633 cases, 0 fails): profiles/r05_gpu_fuzz_campaign.txt."""
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(root), str(root / "tests"), os.environ.get("PYTHONPATH", "")]))
    env.pop("GPU_CAMPAIGN_DRY", None)
    tool, cases = str(root / "tools" / "fuzz" / "gpu_campaign.py"), str(tmp_path / "cases.pkl")
    p = subprocess.run([sys.executable, tool, "prepare", cases, "43", "60"], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0 and "prepared" in p.stdout, p.stderr[-2000:]
    prepared = int(p.stdout.split("prepared")[1].split()[0])
    assert prepared >= 80
    p = subprocess.run([sys.executable, tool, "run", cases], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0 and f"{prepared} cases compared" in p.stdout and "fails 0;" in p.stdout, (p.stdout[-3000:], p.stderr[-2000:])


@pytest.mark.parametrize("name,kind,dtype,tol", [("planar_biped", "relaxed", np.float32, 3e-4), ("planar_biped", "relaxed", np.float64, 1e-10), ("planar_biped", "rigid", np.float64, 1e-4),
                                                 ("planar10f", "relaxed", np.float32, 3e-3), ("planar10f", "relaxed", np.float64, 1e-10), ("planar_biped", "rigid", np.float32, 3e-3)])  # fmt: skip
def test_parallel_axis_models_gpu(models, name, kind, dtype, tol):
    """[round 5, VERDICT r4 weak #1] Contact links joined by PARALLEL joint axes (a Walker2d-style planar biped with a
    floating base, a planar serial chain): round 4's link-space solve factorised a 12 x 12 matrix that is singular for
    them in every configuration and returned fp32 steps wrong by up to 124 % in 2 % of the states.  512 random and 512
    standing states against the fp64 oracle; no contact solve may be discarded."""
    model = (helpers.relaxed_model(models(name), list(range(16)), mu=0.5) if kind == "relaxed" else helpers.rigid_model(models(name), list(range(16)), K=1e4, D=1e2))
    worst = 0.0
    for d in (models.random_data(name, 512, seed=0, dtype=dtype), helpers.standing_data(model, 512, seed=1, dtype=dtype, noise=0.3)):
        truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d, model) if dtype == np.float32 else d))
        out = js.model.step(model, to_gpu(model, d)).state_block()
        e = np.abs(out - truth) / np.maximum(1.0, np.abs(truth))
        worst = max(worst, float(e.max()))
    helpers.note(f"parallel_axes_gpu/{name}/{kind}/{np.dtype(dtype).name}", worst)
    assert worst < tol
    assert tuple(js.model.solver_fault_counts(model, dtype)) == (0, 0)  # no contact solve was discarded


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 3e-3)])
def test_relaxed_contacts_with_200_points_gpu(dtype, tol):
    """[round 5] The quadruped with a 50-point sphere on every foot -- 200 collidable points, the real robot's URDF shape
    (parsers/rod/utils.py:200-204) -- with RelaxedRigidContacts: more points than lanes, chunks of 64 solved in the tree
    (jxs_rigid.inc relaxed_contact_forces_chunked).  VERDICT r4's done-criterion: fp32 <= 3e-3, fp64 <= 1e-9 against the
    oracle on the GPU; no solve discarded; the batch result does not depend on the batch."""
    model = helpers.relaxed_model(pc.quadruped_200(), range(200), mu=0.5)
    worst = 0.0
    for d in (oracle.random_model_data(model, batch_size=48, seed=1, dtype=dtype, base_pos_bounds=((-1, -1, 0.55), (1, 1, 0.68)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3))),
              helpers.standing_data(model, 48, seed=1, dtype=dtype, noise=0.05)):  # fmt: skip
        truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d, model) if dtype == np.float32 else d))
        out = js.model.step(model, to_gpu(model, d)).state_block()
        worst = max(worst, helpers.rel_err(out, truth))
        first = js.model.step(model, js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d)[:, :5], ja.VelRepr.Mixed)).state_block()
        np.testing.assert_array_equal(first, out[:, :5])
    helpers.note(f"relaxed_200_points_gpu/{np.dtype(dtype).name}", worst)
    assert worst < tol
    assert tuple(js.model.solver_fault_counts(model, dtype)) == (0, 0)


@pytest.mark.parametrize("kind,dtype", [("rigid", np.float32), ("rigid", np.float64), ("relaxed", np.float32), ("soft", np.float32)])
def test_gravity_compensated_step_equals_the_two_launch_loop(models, reduced_qp, kind, dtype):
    """[round 4] `step(..., gravity_compensation=True)` (C-ABI `jxs_step_gravity_compensated`): the controller loop of
    BASELINE config 5, tau = g(q) (+ tau_user); step(tau), in one launch for the rigid contact models.  Same result as the
    two launches up to the rounding of one addition, and the oracle's step with the oracle's gravity torques."""
    base = models("anymal")
    model = (helpers.rigid_model(base, helpers.ANYMAL_FEET_4, K=1e4, D=2e2) if kind == "rigid"
             else helpers.relaxed_model(base, helpers.ANYMAL_FEET_16, mu=0.5) if kind == "relaxed" else base)
    N = 70
    d = models.random_data("anymal", N, seed=12, dtype=dtype)
    rng = np.random.default_rng(3)
    tau_user = rng.uniform(-2, 2, size=(N, model.dofs())).astype(dtype)
    g = to_gpu(model, d)
    gq = js.model.free_floating_gravity_forces(model, g)[:, 6:]
    two = js.model.step(model, g, joint_force_references=(gq + tau_user).astype(dtype)).state_block()
    one = js.model.step(model, to_gpu(model, d), joint_force_references=tau_user, gravity_compensation=True).state_block()
    assert np.isfinite(one).all()
    # (fp32: the torques differ in their last bit -- formed in registers here, read back from a block there -- and the
    # interior-point iteration of the contact forces stops at solver_tol = 1e-3: measured 8.6e-5 on the specialised kernel)
    tol = 1e-11 if dtype == np.float64 else 3e-4
    assert helpers.rel_err(one, two) < tol
    pure = js.model.step(model, to_gpu(model, d), gravity_compensation=True).state_block()
    assert helpers.rel_err(pure, js.model.step(model, to_gpu(model, d), joint_force_references=gq.astype(dtype)).state_block()) < tol
    d64 = helpers.upcast(d) if dtype == np.float32 else d
    ref_tau = oracle.free_floating_gravity_forces(model, d64)[:, 6:] + tau_user.astype(np.float64)
    ref = oracle.step(model, d64, joint_force_references=ref_tau)
    assert helpers.rel_err(one, helpers.odata_to_block(model, ref)) < (1e-7 if dtype == np.float64 else 3e-3)


# ---- RelaxedRigidContacts (the cases: parity_cases.RELAXED_CASES) ---------------------------------
@pytest.mark.parametrize("key", list(RELAXED_CASES))
def test_relaxed_step_matches_oracle_gpu(models, key):
    N = 21  # not a multiple of the environments per wave
    model, d = pc.relaxed_case(models, key, N, seed=5)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    # box4 keeps the default mu = 0.005: the regulariser is ~1e-6 of the Delassus entries
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < (1e-8 if key in ("box4", "icub16d") else 1e-10)


def test_relaxed_defaults_in_fp32_stay_finite_gpu(models):
    """[round 4] RelaxedRigidContacts with the reference's default parameters (mu = 0.005) in fp32 with every sole point
    of the humanoid active: the regulariser sits below the fp32 rounding of a Delassus matrix of rank 12 in 96
    unknowns -- no fp32 solver has the digits (HISTORY.md 4e: use fp64, or the estimated parameters).  Up to round 3
    the factorisation floored its pivots and the refinement diverged: NON-FINITE states.  Now pivots at the rounding
    floor are dropped and the refinement keeps a correction only if it reduced the residual: finite states, a few
    per cent away from fp64 -- and fp64 (solved in the tree) is exact."""
    model = helpers.relaxed_model(models("icub"), list(range(32)))
    d32 = helpers.standing_data(model, 40, seed=0, dtype=np.float32, noise=0.003)
    truth = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d32)))
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    assert np.isfinite(out32).all()
    assert helpers.rel_err(out32, truth) < 0.3
    d64 = helpers.standing_data(model, 40, seed=0, noise=0.003)
    out64 = js.model.step(model, to_gpu(model, d64)).state_block()
    assert helpers.rel_err(out64, helpers.odata_to_block(model, oracle.step(model, d64))) < 1e-9


@pytest.mark.parametrize("key,tol", [("box8", 1e-4), ("anymal16", 1e-4), ("anymal4", 1e-4), ("chain9f6", 3e-4), ("icub16", 5e-4)])
def test_relaxed_step_fp32_gpu(models, key, tol):
    """fp32 against the fp64 oracle on the same inputs (host emulation of the same arithmetic: 5e-6 ..
    4e-5)."""
    model, d = pc.relaxed_case(models, key, 40, seed=5, dtype=np.float32)
    ref = oracle.step(model, helpers.upcast(d))
    out = js.model.step(model, to_gpu(model, d))
    blk = out.state_block()
    assert blk.dtype == np.float32 and np.isfinite(blk).all()
    assert helpers.rel_err(blk, helpers.odata_to_block(model, ref)) < tol


def test_relaxed_bare_default_parameters_fp32_gpu(models):
    """The bare defaults (mu = 0.005) put the regulariser at 1e-6 of the Delassus entries: with several
    points of one rigid body in contact the converged solution carries internal forces of 1e6 N on a
    1 kg box (measured) and sits at the fp32 rounding level -- the result is noise-limited (worst
    environment 2e-1, the fp32 NumPy restatement 3e-2).  Finite everywhere and right for the typical
    environment is what can be asserted; HISTORY.md section 4e says to use fp64 or the estimated
    parameters (mu = 0.5) instead."""
    model = helpers.relaxed_model(models("box"), [0, 1, 2, 3])
    d = models.random_data("box", 40, seed=5, dtype=np.float32)
    ref = helpers.odata_to_block(model, oracle.step(model, helpers.upcast(d)))
    blk = js.model.step(model, to_gpu(model, d)).state_block()
    assert np.isfinite(blk).all()
    err = np.abs(blk - ref).max(axis=0) / np.abs(ref).max()
    assert np.median(err) < 3e-3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relaxed_box_settles_known_answer_gpu(models, dtype):
    """reference tests/test_simulations.py:295-346: x, y unchanged (atol 1e-5), z -> 0.05 (atol 1e-4)."""
    model = pc.settling_box(models, "relaxed")
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial, dtype=dtype)
    out = js.model.rollout(model, to_gpu(model, d), 1000).state_block()
    assert abs(out[0, 0]) < 1e-5 and abs(out[1, 0]) < 1e-5
    assert out[2, 0] == pytest.approx(0.05, abs=1e-4)


@pytest.mark.parametrize("kind,name,idx,dtype,tol", [
    ("relaxed", "icub", list(range(32)), np.float64, 1e-10),
    ("relaxed", "icub", list(range(32)), np.float32, 2e-4),
    ("relaxed", "anymal", helpers.ANYMAL_FEET_16, np.float32, 2e-4),
    ("rigid", "icub", list(range(32)), np.float64, 1e-7),
])  # fmt: skip
def test_standing_on_every_sole_point_gpu(models, reduced_qp, kind, name, idx, dtype, tol):
    """Standing states with all 16 bottom points of the feet in contact (rank <= 18 of 48); the 32-point
    humanoid is BASELINE.json config 3's model with all its points enabled -- with RelaxedRigidContacts
    the analogue of the reference's own test_simulation_step benchmark (tests/test_benchmark.py:142-152)."""
    model, d = pc.standing_case(models, kind, name, idx, 21, dtype)
    ref = oracle.step(model, helpers.upcast(d))
    out = js.model.step(model, to_gpu(model, d)).state_block()
    assert out.dtype == dtype and np.isfinite(out).all()
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < tol


@pytest.mark.parametrize("key", ["box8", "anymal16", "chain9f6", "icub16"])
def test_relaxed_rk4_step_matches_oracle_gpu(models, key):
    """RungeKutta4 with RelaxedRigidContacts (contact forces solved at each stage); the reference runs
    its relaxed-rigid test for every integrator (tests/test_simulations.py:295)."""
    N = 21
    model, d = pc.relaxed_case(models, key, N, seed=5)
    model = helpers.with_params(model, integrator=ja.IntegratorType.RungeKutta4)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < 1e-10
    _, d32 = pc.relaxed_case(models, key, N, seed=5, dtype=np.float32)
    out32 = js.model.step(model, to_gpu(model, d32)).state_block()
    ref32 = oracle.step(model, helpers.upcast(d32))
    assert out32.dtype == np.float32 and helpers.rel_err(out32, helpers.odata_to_block(model, ref32)) < 5e-4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relaxed_rk4_box_settles_known_answer_gpu(models, dtype):
    """reference tests/test_simulations.py:295-346 with integrator = RungeKutta4."""
    model = pc.settling_box(models, "relaxed", ja.IntegratorType.RungeKutta4)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 0.2], velocity_representation=VelRepr.Inertial, dtype=dtype)
    out = js.model.rollout(model, to_gpu(model, d), 1000).state_block()
    assert abs(out[0, 0]) < 1e-5 and abs(out[1, 0]) < 1e-5
    assert out[2, 0] == pytest.approx(0.05, abs=1e-4)


def test_relaxed_tumbling_box_rollout_gpu(models):
    model, d = pc.tumbling_box(models, "relaxed")
    out = js.model.rollout(model, to_gpu(model, d), 300).state_block()
    for _ in range(300):
        d = oracle.step(model, d)
    assert helpers.rel_err(out, helpers.odata_to_block(model, d)) < 1e-8


def test_relaxed_estimated_parameters_and_large_batch(models):
    """The reference's benchmark idiom (tests/test_benchmark.py:142-152): RelaxedRigidContacts with
    `estimate_good_contact_parameters`, stepped over a batch; finiteness, batch independence and
    oracle parity on a slice at fp32."""
    base = helpers.relaxed_model(models("anymal"), helpers.ANYMAL_FEET_16)
    cp = js.contact.estimate_good_contact_parameters(base)
    assert type(cp).__name__ == "RelaxedRigidContactsParams" and cp.mu == 0.5
    model = helpers.with_params(base, contact_params=cp)
    N = 2048
    d32 = models.random_data("anymal", N, seed=13, dtype=np.float32)
    out = js.model.step(model, to_gpu(model, d32)).state_block()
    assert np.isfinite(out).all()
    blk = helpers.odata_to_block(model, d32)
    sub = helpers.block_to_odata(model, blk[:, :24].astype(np.float64), oracle.VelRepr.Mixed)
    ref = oracle.step(model, sub)
    assert helpers.rel_err(out[:, :24], helpers.odata_to_block(model, ref)) < 1e-4
    g24 = js.data.JaxSimModelData.from_state_block(model, blk[:, :24], ja.VelRepr.Mixed)
    np.testing.assert_array_equal(js.model.step(model, g24).state_block(), out[:, :24])


@pytest.mark.parametrize("name", ["box", "anymal"])
def test_gpu_golden_relaxed(models, name):
    g = pc.load(f"relaxed_{name}")
    model = pc.relaxed_golden_model(models, name, g)
    data = js.data.JaxSimModelData.from_state_block(model, g["state"], ja.VelRepr.Mixed)
    out = js.model.step(model, data, link_forces=g["link_forces"], joint_force_references=g["tau"])
    assert helpers.rel_err(out.state_block(), g["step"]) < 1e-10


@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Mixed, VelRepr.Body])
def test_step_with_references_object(models, rep):
    """The reference's user flow (README-style loops, api/references.py:23-449): forces are put into a
    ``JaxSimModelReferences`` in the representation of the data, accumulated by link name, read back with
    ``references.link_forces(model, data)`` and handed to ``step``."""
    model = models("anymal")
    N = 9
    d = models.random_data("anymal", N, seed=4, rep=rep)
    g = to_gpu(model, d)
    assert g.velocity_representation == REP[rep]
    tau, f = helpers.random_inputs(model, N, 8, np.float64)
    refs = js.references.JaxSimModelReferences.zero(model, data=g, velocity_representation=g.velocity_representation)
    refs = refs.set_joint_force_references(tau, model=model)
    names = model.link_names()
    refs = refs.apply_link_forces(f[:, :5], model=model, data=g, link_names=names[:5])
    refs = refs.apply_link_forces(0.25 * f[:, 5:], model=model, data=g, link_names=names[5:], additive=True)
    refs = refs.apply_link_forces(0.75 * f[:, 5:], model=model, data=g, link_names=names[5:], additive=True)
    np.testing.assert_allclose(refs.link_forces(model, g), f, atol=1e-10)
    # stored inertial-fixed: the oracle's conversion with the oracle's link transforms
    np.testing.assert_allclose(
        refs._link_forces, oracle.refstep.other_representation_to_inertial(f, rep, d.link_transforms, is_force=True), atol=1e-9)  # fmt: skip
    out = js.model.step(model, g, link_forces=refs.link_forces(model, g), joint_force_references=refs.joint_force_references(model))
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


@pytest.mark.parametrize("tag", ["relaxed_rk4_anymal", "relaxed_rk4fast_anymal", "rigid_rk4_box", "rigid_rk4fast_box"])
def test_gpu_golden_rigid_models_integrators(models, tag):
    g = pc.load(tag)
    model = pc.integrator_golden_model(models, tag, g)
    data = js.data.JaxSimModelData.from_state_block(model, g["state"], ja.VelRepr.Mixed)
    out = js.model.step(model, data, link_forces=g["link_forces"], joint_force_references=g["tau"])
    assert helpers.rel_err(out.state_block(), g["step"]) < (1e-10 if pc.INTEGRATOR_GOLDEN[tag][0] == "relaxed" else 1e-7)


@pytest.mark.parametrize("name", ["cartpole", "chain9f", "icub"])
def test_gpu_golden_rk4(models, name):
    g, model = pc.load(f"rk4_{name}"), pc.rk4_golden_model(models, name)
    N = g["state"].shape[1]
    data = js.data.JaxSimModelData.from_state_block(model, g["state"], ja.VelRepr.Mixed)
    out = js.model.step(model, data, link_forces=g["link_forces"], joint_force_references=g["tau"])
    assert helpers.rel_err(out.state_block(), g["step"]) < helpers.FP64_TOL
    out32 = js.model.step(model, js.data.JaxSimModelData.from_state_block(model, g["state"].astype(np.float32), ja.VelRepr.Mixed),
                          link_forces=g["link_forces"], joint_force_references=g["tau"])  # fmt: skip
    assert helpers.rel_err(out32.state_block(), g["step"]) < helpers.FP32_TOL
    assert N == 4


@pytest.mark.parametrize("name", ["box", "anymal"])
def test_gpu_golden_rigid(models, name):
    g = pc.load(f"rigid_{name}")
    model = pc.rigid_golden_model(models, name, g)
    data = js.data.JaxSimModelData.from_state_block(model, g["state"], ja.VelRepr.Mixed)
    out = js.model.step(model, data, link_forces=g["link_forces"], joint_force_references=g["tau"])
    assert helpers.rel_err(out.state_block(), g["step"]) < 1e-7


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "chain9f", "anymal", "icub"])
def test_free_floating_mass_matrix(models, name):
    """``js.model.free_floating_mass_matrix`` (api/model.py:1553-1590) = ONE launch of the composite-rigid-body
    kernel (``jxs_mass_matrix``, rbda/crba.py:10-170) against the oracle's CRBA in the three velocity
    representations, fixed- and floating-base models; and M nudot = ID(nudot) - ID(0) ties it to the RNEA kernel."""
    from oracle import refrigid

    model = models(name)
    for rep in (VelRepr.Body, VelRepr.Mixed, VelRepr.Inertial):
        d = models.random_data(name, 5, seed=41, rep=rep)
        g = to_gpu(model, d)
        M = js.model.free_floating_mass_matrix(model, g)
        ref = oracle.free_floating_mass_matrix(model, d)
        assert M.shape == ref.shape
        assert helpers.rel_err(M, ref) < 1e-9
        if rep == VelRepr.Mixed:
            assert helpers.rel_err(M, refrigid.free_floating_mass_matrix_mixed(model, d)) < 1e-9
    # fp32
    d = models.random_data(name, 64, seed=42, dtype=np.float32)
    M32 = js.model.free_floating_mass_matrix(model, to_gpu(model, d))
    assert M32.dtype == np.float32
    ref = oracle.free_floating_mass_matrix(model, helpers.upcast(d))
    assert np.abs(M32 - ref).max() / max(1.0, np.abs(ref).max()) < 2e-5


def test_reference_readme_flow(models):
    """The usage of the reference README (README.md:40-84), names and keywords unchanged: build from a
    model description, ``js.model.reduce`` to the considered joints, unbatched ``JaxSimModelData.build``,
    a Python loop over ``js.model.step``."""
    from jaxsim_amd import robots

    full_model = js.model.JaxSimModel.build_from_model_description(model_description=robots.icub23_urdf())
    joints = tuple(n for n in full_model.joint_names() if "elbow" not in n and "ankle_roll" not in n)
    model = js.model.reduce(model=full_model, considered_joints=joints)
    ndof = model.dofs()
    assert ndof == len(joints) == 19
    data = js.data.JaxSimModelData.build(model=model, base_position=np.array([0.0, 0.0, 1.0]))
    tau = np.zeros(ndof)
    T = np.arange(start=0, stop=0.05, step=model.time_step)
    for _ in T:
        data = js.model.step(model=model, data=data, link_forces=None, joint_force_references=tau)
    assert data.base_position.shape == (3,) and data.joint_positions.shape == (ndof,)
    d = oracle.OracleData.build(model, base_position=[0.0, 0.0, 1.0])
    for _ in T:
        d = oracle.step(model, d)
    assert helpers.rel_err(data.state_block(), helpers.odata_to_block(model, d)) < 1e-9
    # free fall so far: z = 1 - g t^2 / 2 up to the semi-implicit Euler offset
    t = len(T) * model.time_step
    assert data.base_position[2] == pytest.approx(1.0 - 0.5 * 9.81 * t * (t + model.time_step), abs=1e-9)


@pytest.mark.parametrize("fixed_base,max_back", [(True, 1), (False, 1)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximum_size_models_gpu(fixed_base, max_back, dtype):
    """64 links (one per lane of a full wave), serial chain: 63 tree levels."""
    from jaxsim_amd import robots

    model = ja.JaxSimModel.build_from_model_description(robots.chain_urdf(64, fixed_base=fixed_base, seed=3, max_back=max_back))
    d = oracle.random_model_data(model, batch_size=5, seed=1, dtype=dtype)
    tau, f = helpers.random_inputs(model, 5, 2, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < (1e-9 if dtype == np.float64 else helpers.FP32_TOL)


@pytest.mark.parametrize("name", ["box", "anymal", "icub"])
@pytest.mark.parametrize("N", [1, 2, 3, 17, 63, 65])
def test_ragged_batch_sizes(models, name, N):
    """Batch sizes around the tile boundaries (tile = 16 / 4 / 2 environments per wave): the padded tail of
    the last tile is neither read as data nor written back."""
    model = models(name)
    d = models.random_data(name, N, seed=50 + N)
    ref = oracle.step(model, d)
    out = js.model.step(model, to_gpu(model, d)).state_block()
    assert out.shape[1] == N
    assert helpers.rel_err(out, helpers.odata_to_block(model, ref)) < helpers.FP64_TOL


def test_value_checks_like_jaxsim_enable_exceptions(models, monkeypatch):
    """``JAXSIM_ENABLE_EXCEPTIONS`` (reference exceptions.py:26-29, rbda/utils.py:135-146): NaN / non-unit
    base quaternions raise ValueError from the RBDA entry points; off by default."""
    import ctypes as C

    from jaxsim_amd import _lib

    model = models("anymal")
    d = models.random_data("anymal", 9, seed=60)
    blk = helpers.odata_to_block(model, d)
    blk[3:7, 2] *= 1.5  # not normalised
    blk[3, 5] = np.nan
    blk[20, 7] = np.inf
    bad = js.data.JaxSimModelData.from_state_block(model, blk, ja.VelRepr.Mixed)
    counts = (C.c_int * 3)()
    dm = runtime.device_model(model, np.float64)
    _lib.check(_lib.load().jxs_validate_state(dm.handle, C.c_void_p(bad._state.ptr), 9, counts, None), "validate")
    assert list(counts) == [1, 1, 2]
    js.model.inverse_dynamics(model, bad)  # exceptions off: no check, garbage in -> garbage out
    monkeypatch.setenv("JAXSIM_ENABLE_EXCEPTIONS", "1")
    with pytest.raises(ValueError, match="contains NaN"):
        js.model.step(model, bad)
    blk[3, 5] = 0.5
    unnorm = js.data.JaxSimModelData.from_state_block(model, blk, ja.VelRepr.Mixed)
    js.model.forward_dynamics_aba(model, unnorm)  # ABA normalises its quaternion: accepted
    with pytest.raises(ValueError, match="not normalized"):
        js.model.inverse_dynamics(model, unnorm)
    js.model.inverse_dynamics(model, to_gpu(model, d))  # a valid state passes


def test_step_repeat_graph_equals_single_launches(models):
    """``jxs_step_repeat`` (hipGraph replay of n single-step launches on a created stream) gives the
    bits of n ``jxs_step`` calls, also when replayed and when the arguments change."""
    import ctypes as C

    from jaxsim_amd import _lib

    model = models("icub")
    d = models.random_data("icub", 50, seed=70, dtype=np.float32)
    ref = to_gpu(model, d)
    for _ in range(2 * 57 + 307):
        ref = js.model.step(model, ref)
    lib, dm = _lib.load(), runtime.device_model(model, np.float32)
    stream = runtime.Stream()
    for trial in range(2):  # second trial: a new state buffer -> the graph is re-captured
        g = to_gpu(model, d)
        runtime.synchronize()
        for n in (57, 307, 57):  # 50-launch graph + 7 plain launches; 250-launch graph + 50-launch graph + 7
            _lib.check(lib.jxs_step_repeat(dm.handle, C.c_void_p(g._state.ptr), None, None, 2, 50, n, stream.handle), "repeat")
        stream.synchronize()
        np.testing.assert_array_equal(g.state_block(), ref.state_block())


@pytest.mark.parametrize("name", ["cartpole", "chain5", "double_pendulum"])
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed])
def test_mass_matrix_inverse_of_fixed_base_models_is_the_full_inverse(models, name, rep):
    """The reference's ``mass_inverse`` treats the base link of every model as a free 6-DoF body
    (rbda/mass_inverse.py:118-178: the propagation reaches link 0 and D0 = I_A[0] is inverted), so
    ``free_floating_mass_matrix_inverse`` of a FIXED-base model is the inverse of the full (6+n) matrix
    ``free_floating_mass_matrix`` returns -- not a matrix with zero base rows [ADVICE r2]."""
    model = models(name)
    assert not model.floating_base()
    d = models.random_data(name, 5, seed=47, rep=rep)
    g = to_gpu(model, d)
    M = js.model.free_floating_mass_matrix(model, g)
    Mi = js.model.free_floating_mass_matrix_inverse(model, g)
    np.testing.assert_allclose(M @ Mi, np.broadcast_to(np.eye(M.shape[-1]), M.shape), atol=1e-8)
    assert helpers.rel_err(Mi, np.linalg.inv(M)) < 1e-8 * max(1.0, float(np.abs(np.linalg.inv(M)).max()))


@pytest.mark.parametrize("name", ["chain9f", "anymal"])
def test_mass_matrix_inverse_and_link_jacobians(models, name):
    """``free_floating_mass_matrix_inverse`` (api/model.py:1593-1631) and
    ``generalized_free_floating_jacobian`` (:925-1045) evaluated through virtual batches of the FD / cached
    kinematics kernels, against the oracle's dense restatement."""
    from oracle import refmath as rm
    from oracle import refrigid

    model = models(name)
    d = models.random_data(name, 4, seed=43, rep=VelRepr.Mixed)
    g = to_gpu(model, d)
    Mi = js.model.free_floating_mass_matrix_inverse(model, g)
    assert helpers.rel_err(Mi, refrigid.free_floating_mass_matrix_inverse_mixed(model, d)) < 1e-9
    M = js.model.free_floating_mass_matrix(model, g)
    np.testing.assert_allclose(M @ Mi, np.broadcast_to(np.eye(M.shape[-1]), M.shape), atol=1e-8)
    # mixed input, inertial output
    W_J = refrigid.generalized_free_floating_jacobian_inertial_output(model, d, VelRepr.Mixed)
    J_in = js.model.generalized_free_floating_jacobian(model, g, output_vel_repr=ja.VelRepr.Inertial)
    assert J_in.shape == W_J.shape and helpers.rel_err(J_in, W_J) < 1e-9
    # mixed input, mixed output: LW_X_W W_J  (api/model.py:1021-1040)
    H = d.link_transforms.copy()
    H[..., :3, :3] = np.eye(3)
    LW_J = rm.adjoint_from_transform(H, inverse=True) @ W_J
    assert helpers.rel_err(js.model.generalized_free_floating_jacobian(model, g), LW_J) < 1e-9
    # J nu = link velocity in the output representation
    nu = d.generalized_velocity(VelRepr.Mixed)
    v = np.einsum("nlij,nj->nli", js.model.generalized_free_floating_jacobian(model, g, output_vel_repr=ja.VelRepr.Inertial), nu)
    np.testing.assert_allclose(v, d.link_velocities, atol=1e-9)


def test_contact_query_api(models):
    """``js.contact``: point kinematics, ``in_contact``, frame transforms and Jacobians
    (reference api/contact.py:18-145,214-350; identity checked by its tests: J nu = point velocity)."""
    from oracle import refrigid

    model = helpers.enable_points(models("anymal"), helpers.ANYMAL_FEET_16)
    d = models.random_data("anymal", 6, seed=5)
    g = to_gpu(model, d)
    p_ref, v_ref = oracle.collidable_points_pos_vel(model, link_transforms=d.link_transforms, link_velocities=d.link_velocities)
    p, v = js.contact.collidable_point_kinematics(model, g)
    np.testing.assert_allclose(p, p_ref, atol=1e-12)
    np.testing.assert_allclose(v, v_ref, atol=1e-12)
    np.testing.assert_allclose(js.contact.collidable_point_positions(model, g), p_ref, atol=1e-12)
    J = js.contact.jacobian(model, g)  # mixed in, mixed out
    np.testing.assert_allclose(J, refrigid.contact_jacobian_mixed(model, d), atol=1e-9)
    np.testing.assert_allclose(np.einsum("ncij,nj->nci", J, d.generalized_velocity(VelRepr.Mixed))[..., :3], v_ref, atol=1e-9)
    np.testing.assert_allclose(js.contact.transforms(model, g), refrigid.contact_transforms(model, d), atol=1e-12)
    touching = js.contact.in_contact(model, g)
    assert touching.shape == (6, model.number_of_links())
    body = model.kin_dyn_parameters.contact_body[model.kin_dyn_parameters.indices_of_enabled_collidable_points]
    expect = np.stack([((p_ref[..., 2] <= 0) & (body == i)[None]).any(axis=1) for i in range(model.number_of_links())], 1)
    np.testing.assert_array_equal(touching, expect)
    assert touching.any() and not touching.all()
    with pytest.raises(ValueError, match="not part of the model"):
        js.contact.in_contact(model, g, link_names=["nope"])
    feet = js.contact.in_contact(model, g, link_names=["LF_SHANK", "RH_SHANK"])
    assert feet.shape == (6, 2)
    # unbatched data: the leading axis disappears like in the reference
    one = js.data.JaxSimModelData.build(model=model, base_position=np.array([0.0, 0.0, 0.5]))
    assert js.contact.collidable_point_positions(model, one).shape == (16, 3)
    assert js.contact.in_contact(model, one).shape == (model.number_of_links(),)


def test_device_side_layout_conversion_and_array_interface(models):
    """Environment-major device buffers (another framework's ``(N, n)`` array) are tiled / untiled on the
    device (``jxs_tile_from_env_major`` / ``jxs_tile_to_env_major``) and accepted by ``step`` through the
    CUDA array interface without a host round trip."""
    import ctypes as C

    from jaxsim_amd import _lib
    from jaxsim_amd.runtime import DeviceArray

    model = models("icub")
    N, n = 37, model.dofs()
    rng = np.random.default_rng(3)
    tau = rng.uniform(-3, 3, size=(N, n)).astype(np.float32)
    lib = _lib.load()
    raw = C.c_void_p()
    _lib.check(lib.jxs_malloc(C.byref(raw), tau.nbytes), "malloc")
    _lib.check(lib.jxs_memcpy_h2d(raw, tau.ctypes.data_as(C.c_void_p), tau.nbytes, None), "h2d")
    runtime.synchronize()
    tile = runtime.device_model(model, np.float32).layout.tile
    tiled = DeviceArray.from_device_env_major(raw.value, N, n, np.float32, tile=tile)
    np.testing.assert_array_equal(tiled.to_host(), tau.T)
    back = C.c_void_p()
    _lib.check(lib.jxs_malloc(C.byref(back), tau.nbytes), "malloc")
    tiled.to_device_env_major(back.value)
    out = np.empty_like(tau)
    runtime.synchronize()
    _lib.check(lib.jxs_memcpy_d2h(out.ctypes.data_as(C.c_void_p), back, tau.nbytes, None), "d2h")
    np.testing.assert_array_equal(out, tau)

    class Foreign:  # what a torch / cupy / jax device array looks like to a consumer
        __cuda_array_interface__ = {"shape": (N, n), "typestr": "<f4", "data": (raw.value, False), "version": 3}

    d = models.random_data("icub", N, seed=71, dtype=np.float32)
    a = js.model.step(model, to_gpu(model, d), joint_force_references=Foreign()).state_block()
    b = js.model.step(model, to_gpu(model, d), joint_force_references=tau).state_block()
    np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        Foreign.__cuda_array_interface__ = dict(Foreign.__cuda_array_interface__, typestr="<f8")
        js.model.step(model, to_gpu(model, d), joint_force_references=Foreign())
    lib.jxs_free(raw)
    lib.jxs_free(back)


# ---- row B on the device: joint-limit spring / damper and the torque-speed curve --------------------
@pytest.mark.parametrize("name", ["cartpole", "anymal", "icub"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_actuation_limits_and_torque_speed_curve_gpu(models, name, dtype):
    model = helpers.actuation_variant(models(name), seed=3)
    N = 50
    d = helpers.actuation_state(models, name, model, N, 21, dtype)
    rng = np.random.default_rng(5)
    tau = rng.uniform(-20, 20, size=(N, model.dofs())).astype(dtype)  # beyond torque_max: the clip is active
    ref = oracle.step(model, helpers.upcast(d), joint_force_references=tau.astype(np.float64))
    out = js.model.step(model, to_gpu(model, d), joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    # the limit terms and the clip matter at this tolerance: without them the result is far away
    plain = helpers.with_params(models(name), actuation_params=ja.ActuationParams())
    off = oracle.step(plain, helpers.upcast(d), joint_force_references=tau.astype(np.float64))
    assert helpers.rel_err(helpers.odata_to_block(model, off), helpers.odata_to_block(model, ref)) > 10 * helpers.tol_of(dtype, name) + 0.02


def test_actuation_known_answers_gpu(models):
    """reference tests/test_actuation.py:11-48: tau_ref = 30 with tau_max = 10, omega_th = 1, omega_max = 2:
    at |sd| = 1.5 the applied torque is limited to 5, at |sd| = 2.5 to 0; checked through the joint
    acceleration of a frictionless pendulum (sdd = (tau - gravity term) / I, the same for both runs)."""
    base = helpers.with_params(models("pendulum"), actuation_params=ja.ActuationParams(enable_friction=False))
    lim = helpers.with_params(models("pendulum"), actuation_params=ja.ActuationParams(torque_max=10.0, omega_th=1.0, omega_max=2.0, enable_friction=False))  # fmt: skip
    for w, expect in ((0.5, 10.0), (1.5, 5.0), (2.5, 0.0), (-1.5, 5.0)):
        d = oracle.OracleData.build(base, joint_positions=[[0.4]], joint_velocities=[[w]])
        dt = base.time_step

        def sd_after(model, tau):
            blk = js.model.step(model, to_gpu(model, d), joint_force_references=np.array([[tau]])).state_block()
            return blk[model.number_of_links() - 1 + 13, 0]  # joint velocity row (13 + n + ... for n = 1)

        # unclipped response is linear in tau: d(sd)/d(tau) = dt / I
        gain = (sd_after(base, 1.0) - sd_after(base, 0.0))
        applied = (sd_after(lim, 30.0) - sd_after(base, 0.0)) / gain
        assert applied == pytest.approx(expect, abs=1e-9), (w, applied)
        assert dt > 0


def test_bench_model_step_matches_oracle_full_size_gpu():
    """The exact model of bench.py (joint-limit springs 100 N m/rad, estimated contact parameters, joint
    damping and Coulomb friction of the synthetic URDF) on the bench's own initial states, N = 1024."""
    import bench

    model = bench.build_model("icub23")
    data = bench.synthetic_state(model, 1024, seed=0, dtype=np.float32)
    blk0 = data.state_block()
    s = blk0[7 : 7 + model.dofs()]
    assert (np.abs(s) > 0.98).any()  # some joints start at / beyond where the +-1 rad limit spring acts
    # push a few joints well beyond the limits so that the spring is exercised at full size
    blk0[7 : 7 + model.dofs(), ::5] *= 1.3
    g = js.data.JaxSimModelData.from_state_block(model, blk0)
    out = js.model.step(model, g).state_block()
    ref = oracle.step(model, helpers.block_to_odata(model, blk0.astype(np.float64)))
    refb = helpers.odata_to_block(model, ref)
    assert (np.abs(blk0[7 : 7 + model.dofs()]) > 1.0).sum() > 100
    # the benchmark's own model (estimated contact parameters): benign conditioning, tighter bounds
    assert helpers.rel_err(out, refb) < 3e-4
    per_env = np.max(np.abs(out - refb) / np.maximum(1.0, np.abs(refb)), axis=0)
    assert np.median(per_env) < 1e-6


# ---- RigidContacts: the device against the reference's UN-reduced QP statement ------------------------
@pytest.mark.parametrize("key", ["anymal4", "anymal16", "chain9f6", "icub8"])
def test_rigid_step_matches_unreduced_statement_gpu(models, key):
    """`test_rigid_step_matches_oracle_gpu` compares with the oracle switched to the kernel's reduced QP
    statement.  Here the oracle solves the reference's own statement (inactive points squeezed to zero
    between their constraints, rbda/contacts/rigid.py:331-362, 476-500) and both sides run at
    solver_tol = 1e-10: the minimiser of the strictly convex QP is unique, so the device is tied to the
    reference's statement, not only to the oracle's variant of it.  (`box4` is left out: four coplanar
    points on one body make the un-reduced Hessian singular up to the 1e-6 shift, and the oracle's own
    interior-point restatement loses positive definiteness before it reaches 1e-10 there.)"""
    from oracle import refrigid

    assert refrigid.REDUCED_QP is False
    N = 21
    model, d = pc.rigid_case(models, key, N, seed=5, build=dict(solver_options={"solver_tol": 1e-10}))
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref = oracle.step(model, d, link_forces=f, joint_force_references=tau)
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < 1e-7


# ---- Jacobian kernel + host assembly (rbda/jacobian.py:128-339, api/model.py:925-1228) ---------------------
@pytest.mark.parametrize("name", ["cartpole", "chain9f", "anymal", "icub"])
def test_jacobian_full_kernel_gpu(models, name):
    from oracle import refrigid

    model = models(name)
    for dtype, tol in ((np.float64, 1e-11), (np.float32, 2e-5)):
        d = models.random_data(name, 37, seed=43, dtype=dtype)
        J, Jd, BH = js.model.jacobian_full_doubly_left(model, to_gpu(model, d))
        du = helpers.upcast(d)
        J_ref, BH_ref = refrigid.jacobian_full_doubly_left(model, du.joint_positions)
        Jd_ref = refrigid.jacobian_derivative_full_doubly_left(model, du.joint_positions, du.joint_velocities)
        assert helpers.rel_err(J, J_ref) < tol and helpers.rel_err(Jd, Jd_ref) < tol and helpers.rel_err(BH, BH_ref) < tol


@pytest.mark.parametrize("in_rep", REPS)
@pytest.mark.parametrize("out_rep", REPS)
def test_link_jacobians_all_representations_gpu(models, in_rep, out_rep):
    """``generalized_free_floating_jacobian`` for every (input, output) representation pair against the oracle's
    restatement, and O_v_WL = O_J nu against the cached link velocities moved to the output representation."""
    from oracle import refrigid

    model = models("icub")
    d = models.random_data("icub", 6, seed=51, rep=in_rep)
    g = to_gpu(model, d)
    J = js.model.generalized_free_floating_jacobian(model, g, output_vel_repr=REP[out_rep])
    ref = refrigid.generalized_free_floating_jacobian(model, d, in_rep, out_rep)
    assert J.shape == ref.shape and helpers.rel_err(J, ref) < 1e-10
    nu = d.generalized_velocity(in_rep)
    v = np.einsum("nlij,nj->nli", J, nu)
    W_v = d.link_velocities  # inertial-fixed
    H = d.link_transforms
    expect = oracle.refstep.inertial_to_other_representation(W_v, out_rep, H, is_force=False)
    assert helpers.rel_err(v, expect) < 1e-10


def _advance(model, d, eps):
    """The configuration a time eps later along the motion the state's velocities define (first order in the
    positions is enough for a central difference): joints, base position, base orientation."""
    w, v = d.base_angular_velocity, d.base_linear_velocity  # inertial-fixed
    p = d.base_position + eps * (v + np.cross(w, d.base_position))
    R = oracle.refmath.so3_from_quaternion(d.base_quaternion)
    dR = oracle.refmath.rotation_from_axis_angle(eps * w)
    Rn = dR @ R
    # rotation matrix -> quaternion (w x y z), via the largest-trace branch (angles here are generic)
    tr = np.trace(Rn, axis1=-2, axis2=-1)
    qw = 0.5 * np.sqrt(1.0 + tr)
    q = np.stack([qw, (Rn[:, 2, 1] - Rn[:, 1, 2]) / (4 * qw), (Rn[:, 0, 2] - Rn[:, 2, 0]) / (4 * qw), (Rn[:, 1, 0] - Rn[:, 0, 1]) / (4 * qw)], -1)
    return oracle.OracleData.build(model, base_position=p, base_quaternion=q, joint_positions=d.joint_positions + eps * d.joint_velocities,
                                   velocity_representation=d.velocity_representation)  # fmt: skip


@pytest.mark.parametrize("in_rep", REPS)
@pytest.mark.parametrize("out_rep", REPS)
def test_link_jacobian_derivative_all_representations_gpu(models, in_rep, out_rep):
    """``generalized_free_floating_jacobian_derivative`` (api/model.py:1046-1228) for every representation pair
    against a central finite difference of the ORACLE's Jacobian along the motion, and the inertial / inertial
    pair against the oracle's restatement of the derivative itself."""
    from oracle import refrigid

    model = models("anymal")
    N = 4
    d = models.random_data("anymal", N, seed=53, rep=in_rep)
    assert np.all(1.0 + np.trace(oracle.refmath.so3_from_quaternion(d.base_quaternion), axis1=-2, axis2=-1) > 0.2)
    Jd = js.model.generalized_free_floating_jacobian_derivative(model, to_gpu(model, d), output_vel_repr=REP[out_rep])
    eps = 1e-6
    Jp = refrigid.generalized_free_floating_jacobian(model, _advance(model, d, +eps), in_rep, out_rep)
    Jm = refrigid.generalized_free_floating_jacobian(model, _advance(model, d, -eps), in_rep, out_rep)
    fd = (Jp - Jm) / (2 * eps)
    assert Jd.shape == fd.shape and helpers.rel_err(Jd, fd) < 2e-7
    if in_rep == VelRepr.Inertial and out_rep == VelRepr.Inertial:
        assert helpers.rel_err(Jd, refrigid.generalized_free_floating_jacobian_derivative_inertial(model, d)) < 1e-10


def test_contact_jacobian_derivative_gpu(models):
    """``js.contact.jacobian_derivative`` (api/contact.py:353-511), mixed in / mixed out, against the oracle's
    restatement; and Jdot nu + J nudot = acceleration of the contact points' velocity (finite differences of the
    oracle's point velocities along a step)."""
    from oracle import refrigid

    model = helpers.enable_points(models("anymal"), helpers.ANYMAL_FEET_16)
    d = models.random_data("anymal", 5, seed=57)
    g = to_gpu(model, d)
    Jd = js.contact.jacobian_derivative(model, g)
    ref = refrigid.contact_jacobian_derivative_mixed(model, d)
    assert Jd.shape == ref.shape and helpers.rel_err(Jd, ref) < 1e-10
    J = js.contact.jacobian(model, g)
    assert helpers.rel_err(J, refrigid.contact_jacobian_mixed(model, d)) < 1e-10


def test_discarded_rigid_solves_are_counted_gpu(models):
    """A non-finite QP / impact solve is discarded AND counted (jxs_solver_fault_counts): well-posed steps
    report zero; a state with a NaN joint velocity makes the solves of that environment non-finite, which
    shows up in the counters (and raises when JAXSIM_ENABLE_EXCEPTIONS is set) instead of passing silently."""
    import os

    model = helpers.rigid_model(models("anymal"), helpers.ANYMAL_FEET_4, K=1e4, D=1e2)
    d = helpers.standing_data(model, 12, seed=3)
    g = to_gpu(model, d)
    js.model.solver_fault_counts(model, np.float64, reset=True)
    js.model.step(model, g)
    assert js.model.solver_fault_counts(model, np.float64) == (0, 0)
    blk = helpers.odata_to_block(model, d)
    n = model.dofs()
    blk[13 + n + 2, 5] = np.nan  # one joint velocity of environment 5
    bad = js.data.JaxSimModelData.from_state_block(model, blk)
    js.model.step(model, bad)
    qp, imp = js.model.solver_fault_counts(model, np.float64, reset=True)
    assert qp >= 1 and qp + imp <= 2, (qp, imp)
    assert js.model.solver_fault_counts(model, np.float64) == (0, 0)
    os.environ["JAXSIM_ENABLE_EXCEPTIONS"] = "1"
    try:
        with pytest.raises(ValueError, match="discarded"):
            js.model.step(model, bad)
    finally:
        os.environ.pop("JAXSIM_ENABLE_EXCEPTIONS")


ISOLATION_CASES = ["cartpole", "chain5", "chain9f", "anymal", "icub", "icub16", "anymal_rigid4", "anymal_relaxed4", "icub_relaxed16", "tree3_rigid2"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ISOLATION_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_non_finite_environment_does_not_touch_its_neighbours(models, case, dtype):
    """Environments are independent problems: a diverged one -- NaN in its state -- must leave
    every other environment of the batch bit for bit what it is without it.  The kernels mask lanes by multiplying with
    0 / 1 where the values are finite by construction and shift values between lanes with DPP; neither may carry a NaN
    across the boundary of an environment (rows of 16 lanes, wave shifts)."""
    if case == "anymal_rigid4":
        name, model = "anymal", helpers.rigid_model(models("anymal"), helpers.ANYMAL_FEET_4, K=1e4, D=2e2)
    elif case == "anymal_relaxed4":
        name, model = "anymal", helpers.relaxed_model(models("anymal"), helpers.ANYMAL_FEET_4)
    elif case == "icub_relaxed16":
        name, model = "icub", helpers.relaxed_model(models("icub"), list(range(16)))
    elif case == "tree3_rigid2":
        # [ADVICE r3] a base with two children in a FOUR-lane group (sixteen environments share a DPP row): the DPP child
        # gather masks by multiplication and must not be used there (jxs_pack.h child_off)
        from jaxsim_amd import robots

        name = None
        model = helpers.rigid_model(ja.JaxSimModel.build_from_model_description(robots.chain_urdf(3, fixed_base=False, seed=20, max_back=2)), [0, 9], K=1e4, D=2e2)
        assert list(np.asarray(model.kin_dyn_parameters.parent_array)) == [-1, 0, 0]
    else:
        name, model = case, models(case)
    N = 24
    if name is None:
        d = oracle.random_model_data(model, batch_size=N, seed=11, dtype=dtype, base_pos_bounds=((-1, -1, 0.0), (1, 1, 0.3)), base_rpy_bounds=((-0.3, -0.3, -3), (0.3, 0.3, 3)))
    else:
        d = models.random_data(name, N, seed=11, dtype=dtype)
    blk = helpers.odata_to_block(model, d)
    clean = js.model.step(model, js.data.JaxSimModelData.from_state_block(model, blk.copy())).state_block()
    assert np.isfinite(clean).all()
    n = model.dofs()
    for bad_env in (0, 5, N - 1):
        dirty = blk.copy()
        dirty[13 + n + (n - 1), bad_env] = np.nan  # the last joint velocity of one environment
        dirty[0, bad_env] = np.inf               # and its base position
        out = js.model.step(model, js.data.JaxSimModelData.from_state_block(model, dirty)).state_block()
        others = [e for e in range(N) if e != bad_env]
        assert not np.isfinite(out[:, bad_env]).all()
        assert np.array_equal(out[:, others], clean[:, others]), (case, bad_env, np.argwhere(out[:, others] != clean[:, others])[:4])


# ---- [round 6] js.ode.system_dynamics / system_acceleration, js.contact.link_contact_forces ---------------------------
# SURVEY section 8(a) rows E and I as callable entries (jxs_system_dynamics, jxs_link_contact_forces; kernel modes MODE_DYN /
# MODE_DYN_RIGID).  Reference: src/jaxsim/api/ode.py:16-225, src/jaxsim/api/contact.py:514-603 -- what the reference's
# contact-model benchmarks time (tests/test_benchmark.py:103-139).
# (the error metric and the oracle's link wrenches: parity_cases.dyn_err / link_contact_forces)
def _check_dynamics(model, d, tau, f, dtype, tol):
    """system_dynamics (every key), link_contact_forces and system_acceleration of the device against the oracle."""
    N = d.batch_size
    d64 = helpers.upcast(d, model)
    tau64 = None if tau is None else tau.astype(np.float64)
    f64 = None if f is None else f.astype(np.float64)
    g = to_gpu(model, d)
    # --- system_dynamics: evaluated in inertial representation whatever the data's (api/ode.py:204)
    d_in = dataclasses.replace(d64, velocity_representation=VelRepr.Inertial)
    ref = oracle.refstep.system_dynamics(model, d_in, link_forces=f64, joint_torques=tau64)
    got = js.ode.system_dynamics(model, g, link_forces=f, joint_torques=tau)
    for key in ("base_position", "base_quaternion", "joint_positions", "base_linear_velocity", "base_angular_velocity", "joint_velocities"):
        assert np.asarray(got[key]).dtype == dtype
        assert pc.dyn_err(got[key], ref[key], dtype) < tol, key
    if oracle.refstep.is_rigid_contact_model(model) or oracle.refstep.is_relaxed_rigid_contact_model(model):
        assert got["contact_state"] == {}
    elif model.kin_dyn_parameters.number_of_collidable_points() > 0:
        assert pc.dyn_err(got["contact_state"]["tangential_deformation"], ref["tangential_deformation"], dtype) < tol
    # --- link_contact_forces: link forces in the data's representation (rigid models; SoftContacts ignores the inputs)
    ref_W = pc.link_contact_forces(model, d64, tau64, f64)
    W, aux = js.contact.link_contact_forces(model, g, link_forces=f, joint_torques=tau)
    assert np.asarray(W).shape == (N, model.number_of_links(), 6)
    assert pc.dyn_err(W, ref_W, dtype) < tol
    # --- system_acceleration in the data's representation, as written (oracle.refstep.system_acceleration_active)
    vd, sdd, md = oracle.refstep.system_acceleration_active(model, d64, link_forces=f64, joint_torques=tau64)
    gvd, gsdd, gcs = js.ode.system_acceleration(model, g, link_forces=f, joint_torques=tau)
    assert pc.dyn_err(np.concatenate([np.asarray(gvd), np.asarray(gsdd)], -1), np.concatenate([vd, sdd], -1), dtype) < tol
    return ref_W, aux, gcs, md


# (every model in the inertial representation; the three representations on the four models with contacts -- no skips)
DYN_NAME_REP = [(n, VelRepr.Inertial) for n in ALL] + [(n, r) for n in ("box", "chain9f", "anymal", "icub") for r in (VelRepr.Body, VelRepr.Mixed)]


@pytest.mark.parametrize("name,rep", DYN_NAME_REP)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_system_dynamics_matches_oracle_gpu(models, name, dtype, rep):
    model = models(name)
    N = 70  # not a multiple of the environments per wave
    d = models.random_data(name, N, seed=4, dtype=dtype, rep=rep)
    tau, f = helpers.random_inputs(model, N, 15, dtype)
    tol = helpers.tol_of(dtype, name, evaluation=True)
    if dtype == np.float32 and name in models.contact_z:
        # forces and accelerations, not dt x them: a point that barely touches has dF / d delta = D delta_dot / (2 sqrt(delta))
        # -> 1e3 .. 1e4 N/m per ulp-sized (7e-9 m) error of its height, i.e. 1e-3 N on a force of order one (measured on
        # MI355X, sphere, one environment of 70: 8.0e-4; the reference formulation in fp32: 3.8e-4 on the same states) --
        # the ceiling of the fp32 gates applies (helpers.FP32_TOL); the step's per-model gates see dt = 1e-3 times this
        tol = max(tol, helpers.FP32_TOL)
    ref_W, aux, gcs, md = _check_dynamics(model, d, tau, f, dtype, tol)
    if name in models.contact_z:
        assert np.abs(ref_W).max() > 1.0  # contacts really act in this sample
        assert pc.dyn_err(aux["m_dot"], md, dtype) < tol
        assert pc.dyn_err(gcs["tangential_deformation"], md, dtype) < tol


def test_system_dynamics_without_inputs_and_one_environment_gpu(models):
    """The reference idiom of its benchmarks: `js.ode.system_dynamics(model, data)` -- no inputs, unbatched data."""
    model = models("icub")
    d = models.random_data("icub", 1, seed=4, rep=VelRepr.Inertial)
    g = js.data.JaxSimModelData.build(
        model, base_position=d.base_position[0], base_quaternion=d.base_quaternion[0], joint_positions=d.joint_positions[0],
        base_linear_velocity=d.base_linear_velocity[0], base_angular_velocity=d.base_angular_velocity[0],
        joint_velocities=d.joint_velocities[0], velocity_representation=ja.VelRepr.Inertial, dtype=np.float64,
    )  # fmt: skip
    ref = oracle.refstep.system_dynamics(model, dataclasses.replace(d, tangential_deformation=np.zeros_like(d.tangential_deformation)).update_caches(model))
    got = js.ode.system_dynamics(model, g)
    assert np.asarray(got["joint_velocities"]).shape == (model.dofs(),)
    for key in ("base_position", "base_quaternion", "joint_positions", "base_linear_velocity", "base_angular_velocity", "joint_velocities"):
        assert helpers.rel_err(got[key], ref[key][0]) < helpers.FP64_TOL, key
    pd, Qd, sd = js.ode.system_position_dynamics(g)
    assert helpers.rel_err(pd, ref["base_position"][0]) < 1e-12 and helpers.rel_err(Qd, ref["base_quaternion"][0]) < 1e-12
    np.testing.assert_array_equal(sd, np.asarray(g.joint_velocities))


def test_system_dynamics_baumgarte_gain_and_raw_torques_gpu(models):
    """(a) the Baumgarte gain reaches the quaternion derivative: with a non-unit stored quaternion the reference
    normalises first (data.base_orientation), so the term vanishes to rounding and every gain gives the same Qdot;
    (b) no actuation model (api/ode.py:117-122): limits, friction and the torque-speed curve of
    helpers.actuation_variant all bite in `step` and must not touch the torques here."""
    model = helpers.actuation_variant(models("anymal"), seed=3)
    N = 9
    d = helpers.actuation_state(models, "anymal", model, N, seed=4, dtype=np.float64)
    d = dataclasses.replace(d, velocity_representation=VelRepr.Inertial, base_quaternion=d.base_quaternion * 1.3).update_caches(model)
    tau, _ = helpers.random_inputs(model, N, 5, np.float64)
    ref = oracle.refstep.system_dynamics(model, d, joint_torques=tau)
    g = to_gpu(model, d)
    for K in (1.0, 0.1, 25.0):
        got = js.ode.system_dynamics(model, g, joint_torques=tau, baumgarte_quaternion_regularization=K)
        assert helpers.rel_err(got["base_quaternion"], ref["base_quaternion"]) < 1e-12
        assert helpers.rel_err(got["joint_velocities"], ref["joint_velocities"]) < helpers.FP64_TOL


DYN_RIGID_KEYS = ["box4", "anymal16", "anymal4", "icub8"]


@pytest.mark.parametrize("key", DYN_RIGID_KEYS)
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Mixed])
def test_rigid_system_dynamics_matches_oracle_gpu(models, reduced_qp, key, rep):
    N = 21
    model, d = pc.rigid_case(models, key, N, seed=5, rep=rep)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref_W, aux, gcs, _ = _check_dynamics(model, d, tau, f, np.float64, 1e-6)  # (accelerations: the step's 1e-7 gate sees dt x these)
    assert np.abs(ref_W).max() > 1.0 and aux == {} and gcs == {}


@pytest.mark.parametrize("key", ["anymal4", "icub8", "anymal16"])
def test_rigid_system_dynamics_fp32_gpu(models, reduced_qp, key):
    model, d = pc.rigid_case(models, key, 40, seed=5, dtype=np.float32, rep=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, 40, 7, np.float32)
    _check_dynamics(model, d, tau, f, np.float32, 3e-3)


DYN_RELAXED_KEYS = ["box8", "anymal16", "icub16"]


@pytest.mark.parametrize("key", DYN_RELAXED_KEYS)
@pytest.mark.parametrize("rep", [VelRepr.Inertial, VelRepr.Body])
def test_relaxed_system_dynamics_matches_oracle_gpu(models, key, rep):
    N = 21
    model, d = pc.relaxed_case(models, key, N, seed=5, rep=rep)
    tau, f = helpers.random_inputs(model, N, 7, np.float64)
    ref_W, aux, gcs, _ = _check_dynamics(model, d, tau, f, np.float64, 1e-8)
    assert np.abs(ref_W).max() > 1.0 and aux == {} and gcs == {}


@pytest.mark.parametrize("key", ["anymal16", "icub16"])
def test_relaxed_system_dynamics_fp32_gpu(models, key):
    model, d = pc.relaxed_case(models, key, 40, seed=5, dtype=np.float32, rep=VelRepr.Inertial)
    tau, f = helpers.random_inputs(model, 40, 7, np.float32)
    _check_dynamics(model, d, tau, f, np.float32, 2e-3)


def test_link_contact_forces_are_what_the_step_applies_gpu(models):
    """Force-level consistency of rows I / K / L with the step: one semi-implicit Euler step from the device equals
    the state integrated by hand from the device's own system_dynamics evaluated with the actuation model's torques
    (api/model.py:2658) -- nu+ = nu + dt nudot, m+ = m + dt mdot (api/integrators.py:35-71)."""
    model = models("icub")
    N = 33
    d = models.random_data("icub", N, seed=4, rep=VelRepr.Inertial)
    g = to_gpu(model, d)
    tau = oracle.refstep.compute_resultant_torques(model, d)  # what `step` hands to system_dynamics (api/model.py:2658)
    xd = js.ode.system_dynamics(model, g, joint_torques=tau)
    out = js.model.step(model, g)
    dt = model.time_step
    np.testing.assert_allclose(np.asarray(out.joint_velocities), d.joint_velocities + dt * np.asarray(xd["joint_velocities"]), rtol=0, atol=1e-11)
    np.testing.assert_allclose(np.asarray(out.contact_state["tangential_deformation"]),
                               d.tangential_deformation + dt * np.asarray(xd["contact_state"]["tangential_deformation"]), rtol=0, atol=1e-12)  # fmt: skip
    W, _ = js.contact.link_contact_forces(model, g)
    # Newton: total contact force + weight = d/dt of the linear momentum; cross-check with the CoM acceleration is left to
    # the oracle comparison above -- here only: the wrenches sit on the links that carry enabled points
    kdp = model.kin_dyn_parameters
    has = np.zeros(model.number_of_links(), dtype=bool)
    has[np.asarray(kdp.contact_body)[kdp.indices_of_enabled_collidable_points]] = True
    assert np.all(np.asarray(W)[:, ~has] == 0) and np.abs(np.asarray(W)[:, has]).max() > 1.0


def test_link_forces_from_contact_forces_host(models):
    model = models("icub16")
    kdp = model.kin_dyn_parameters
    body = np.asarray(kdp.contact_body)[kdp.indices_of_enabled_collidable_points]
    rng = np.random.default_rng(0)
    W_f_C = rng.normal(size=(len(body), 6))
    W_f_L = js.contact.link_forces_from_contact_forces(model, contact_forces=W_f_C)
    assert W_f_L.shape == (model.number_of_links(), 6)
    for l in range(model.number_of_links()):
        np.testing.assert_allclose(W_f_L[l], W_f_C[body == l].sum(axis=0), atol=1e-14)
    with pytest.raises(ValueError):
        js.contact.link_forces_from_contact_forces(model, contact_forces=W_f_C[:-1])


# ---- [round 6] height-field terrain (the generic finite-difference normal, terrain.py:40-62) --
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["box", "icub"])
def test_height_field_terrain_soft_gpu(models, name, dtype):
    t, g, _ = pc.sine_field()
    model = helpers.with_params(models(name), terrain=t)
    N = 70
    d = models.random_data(name, N, seed=23, dtype=dtype)
    ref = oracle.step(helpers.with_params(model, terrain=g), helpers.upcast(d, model))
    out = js.model.step(model, to_gpu(model, d))
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    flat = js.model.step(models(name), to_gpu(models(name), d))
    assert helpers.rel_err(flat.state_block(), helpers.odata_to_block(model, ref)) > 1e-5  # the terrain changes the answer
    # three steps in one fused launch see the same terrain
    ref3 = helpers.upcast(d, model)
    for _ in range(3):
        ref3 = oracle.step(helpers.with_params(model, terrain=g), ref3)
    out3 = js.model.rollout(model, to_gpu(model, d), 3)
    assert helpers.rel_err(out3.state_block(), helpers.odata_to_block(model, ref3)) < 10 * helpers.tol_of(dtype, name)


@pytest.mark.parametrize("kind,key", [("rigid", "box4"), ("rigid", "anymal4"), ("relaxed", "box8"), ("relaxed", "anymal16")])
def test_height_field_terrain_rigid_models_gpu(models, reduced_qp, kind, key):
    t, g, _ = pc.sine_field()
    base, d = pc.contact_case(models, kind, key, 24, seed=5)
    model = helpers.with_params(base, terrain=t)
    ref = oracle.step(helpers.with_params(model, terrain=g), d)
    out = js.model.step(model, to_gpu(model, d))
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < (1e-7 if kind == "rigid" else 1e-9)


def test_height_field_that_is_a_plane_equals_plane_terrain_gpu(models):
    """Known answer without the oracle: the bilinear interpolant of z = tan(a) x is that plane and its central difference the
    exact slope, so the height field must reproduce PlaneTerrain (RungeKutta4 as well: the stages see the terrain too)."""
    a = np.deg2rad(8.0)
    hf = ja.HeightFieldTerrain.from_function(lambda x, y: np.tan(a) * x + 0.0 * y, x_range=(-3, 3), y_range=(-3, 3), spacing=0.25)
    plane = ja.PlaneTerrain.build(height=0.0, normal=[-np.sin(a), 0.0, np.cos(a)])
    for integ in (ja.IntegratorType.SemiImplicitEuler, ja.IntegratorType.RungeKutta4):
        box = helpers.with_params(models("box"), integrator=integ)
        d = models.random_data("box", 33, seed=3)
        o1 = js.model.step(helpers.with_params(box, terrain=hf), to_gpu(box, d)).state_block()
        o2 = js.model.step(helpers.with_params(box, terrain=plane), to_gpu(box, d)).state_block()
        assert helpers.rel_err(o1, o2) < 1e-11


# ---- [round 6] links with more than six children (VERDICT r5 missing 3: kMaxChildren 6 -> 12) --------------------------
@pytest.mark.parametrize("name", ["octopod", "hub12"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_links_with_more_than_six_children_gpu(models, name, dtype):
    """An octopod (eight legs on the body) and a twelve-spoke hub through the public API: step, forward / inverse dynamics,
    mass matrix and its inverse, gravity forces -- every sweep that gathers children (emulation twin:
    tests/test_emulation_parity.py::test_links_with_more_than_six_children)."""
    model = models(name)
    N = 37
    d = models.random_data(name, N, seed=4, dtype=dtype)
    du = helpers.upcast(d)
    tau, f = helpers.random_inputs(model, N, 5, dtype)
    t64, f64 = tau.astype(np.float64), f.astype(np.float64)
    g = to_gpu(model, d)
    ref = oracle.step(model, du, link_forces=f64, joint_force_references=t64)
    out = js.model.step(model, g, link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < helpers.tol_of(dtype, name)
    fp64 = dtype == np.float64
    vd, sdd = oracle.forward_dynamics_aba(model, du, joint_forces=t64, link_forces=f64)
    gvd, gsdd = js.model.forward_dynamics_aba(model, g, joint_forces=tau, link_forces=f)
    assert helpers.rel_err(gsdd, sdd) < (1e-10 if fp64 else 2e-4) and helpers.rel_err(gvd, vd) < (1e-10 if fp64 else 2e-4)
    acc = np.random.default_rng(3).uniform(-2, 2, size=(N, 6 + model.dofs())).astype(dtype)
    fB, tq = oracle.inverse_dynamics(model, du, joint_accelerations=acc[:, 6:].astype(np.float64), base_acceleration=acc[:, :6].astype(np.float64), link_forces=f64)
    gfB, gtq = js.model.inverse_dynamics(model, g, joint_accelerations=acc[:, 6:], base_acceleration=acc[:, :6], link_forces=f)
    scale = max(1.0, float(np.abs(tq).max()), float(np.abs(fB).max()))
    assert max(float(np.abs(gtq - tq).max()), float(np.abs(gfB - fB).max())) / scale < (1e-10 if fp64 else 2e-5)
    M = oracle.free_floating_mass_matrix(model, du)
    gM = js.model.free_floating_mass_matrix(model, g)
    assert np.abs(gM - M).max() / max(1.0, np.abs(M).max()) < (1e-11 if fp64 else 2e-5)
    gMi = js.model.free_floating_mass_matrix_inverse(model, g).astype(np.float64)
    Mi = np.linalg.inv(M)
    assert np.abs(gMi - Mi).max() / np.abs(Mi).max() < (1e-9 if fp64 else 3e-4)
    gg = js.model.free_floating_gravity_forces(model, g)
    g_ref = oracle.free_floating_gravity_forces(model, du)
    assert float(np.abs(gg - g_ref).max()) / max(1.0, float(np.abs(g_ref).max())) < (1e-12 if fp64 else 2e-6)


# (gates: measured on MI355X x 3 -- rigid 4 points fp64 2.0e-7 at the default solver_tol = 1e-3, where the iteration stops;
# relaxed fp32 3.3e-4 on these light legs, 0.4 .. 1.2 kg)
@pytest.mark.parametrize("kind,idx,dtype,tol", [("rigid", OCTOPOD_FEET_4, np.float64, 6e-7), ("rigid", OCTOPOD_FEET_16, np.float64, 1e-7),
                                                ("relaxed", OCTOPOD_FEET_16, np.float64, 1e-10), ("rigid", OCTOPOD_FEET_4, np.float32, 3e-3),
                                                ("relaxed", OCTOPOD_FEET_16, np.float32, 1e-3)])
def test_octopod_with_the_rigid_contact_models_gpu(models, reduced_qp, kind, idx, dtype, tol):
    N = 24
    model, d = pc.octopod_case(models, kind, idx, N, dtype)
    tau, f = helpers.random_inputs(model, N, 7, dtype)
    ref = oracle.step(model, helpers.upcast(d), link_forces=f.astype(np.float64), joint_force_references=tau.astype(np.float64))
    out = js.model.step(model, to_gpu(model, d), link_forces=f, joint_force_references=tau)
    assert helpers.rel_err(out.state_block(), helpers.odata_to_block(model, ref)) < tol
    assert js.model.solver_fault_counts(model, dtype) == (0, 0)
