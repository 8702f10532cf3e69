"""Centroidal momentum, CoM and energies on the GPU (``js.com``, ``js.model`` momentum / energy functions, ``jxs_centroidal``).

3. Every new function against the reference's definitions (tests/centroidal_ref.py) in the three velocity
   representations and both ``output_vel_repr`` paths; fp64 1e-10, fp32 with per-model gates; N = 1 and N not a multiple
   of the tile.
4. Device self-consistency: total_momentum_jacobian = free_floating_mass_matrix[:6], 2 K = nu^T M nu (device M).
5. Oracle-free physics on trajectories without contact: finite difference of the CoM, momentum in RungeKutta4 free
   flight, K - U of a fixed-base chain under RungeKutta4.
6. The device-resident extension ``js.com.centroidal_quantities``.
7. Library kernel against the model-specialised kernel of MODE_CENTROIDAL.
"""
import numpy as np
import pytest

import centroidal_ref as cr
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
from jaxsim_amd import runtime, specialize
from jaxsim_amd.runtime import DeviceArray
from oracle import VelRepr

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)
_JREP = {VelRepr.Inertial: ja.VelRepr.Inertial, VelRepr.Body: ja.VelRepr.Body, VelRepr.Mixed: ja.VelRepr.Mixed}
NAMES = ["anymal", "icub", "cartpole", "chain5", "box", "octopod"]
# fp32 gates per model (tests/helpers.py style: measured worst x ~3); the average-velocity quantities solve with I_G and
# carry its condition number -- the cart-pole's slender pole: measured worst 4.7e-4 (average_velocity_jacobian, Inertial)
FP32_TOL = {"anymal": 2e-5, "icub": 2e-5, "cartpole": 2e-5, "chain5": 2e-5, "box": 2e-5, "octopod": 2e-5}
FP32_TOL_AVG = {"cartpole": 1.5e-3}
FLIGHT_STEPS = 200


def free_flight_model(zoo):
    """Floating chain, RungeKutta4, no friction (nothing but gravity acts in the air)."""
    return helpers.with_params(zoo("chain9f"), integrator=ja.IntegratorType.RungeKutta4,
                               actuation_params=ja.ActuationParams(enable_friction=False))  # fmt: skip


def fixed_chain_model(zoo):
    return helpers.with_params(zoo("double_pendulum"), integrator=ja.IntegratorType.RungeKutta4,
                               actuation_params=ja.ActuationParams(enable_friction=False))  # fmt: skip


def gpu_models(zoo):
    """Every model this module launches (``__graft_entry__.prebuild_specialised`` builds their kernels)."""
    return [zoo(n) for n in NAMES] + [free_flight_model(zoo), fixed_chain_model(zoo)]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


def device_data(model, d, rep, dtype):
    return js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d, dtype=dtype), _JREP[rep])


def functional(model, data, rep):
    """Every new function, as the user calls them; ``*_out``: per output representation."""
    out = {f: getattr(js.com, f)(model, data) for f in (
        "com_position", "com_linear_velocity", "centroidal_momentum", "centroidal_momentum_jacobian",
        "locked_centroidal_spatial_inertia", "average_centroidal_velocity", "average_centroidal_velocity_jacobian")}  # fmt: skip
    out.update({f: getattr(js.model, f)(model, data) for f in (
        "total_momentum", "locked_spatial_inertia", "average_velocity", "kinetic_energy", "potential_energy",
        "mechanical_energy")})  # fmt: skip
    out["total_momentum_jacobian_out"] = {o: js.model.total_momentum_jacobian(model, data, output_vel_repr=_JREP[o]) for o in REPS}
    out["average_velocity_jacobian_out"] = {o: js.model.average_velocity_jacobian(model, data, output_vel_repr=_JREP[o]) for o in REPS}
    out["link_spatial_inertia_matrices"] = js.model.link_spatial_inertia_matrices(model)
    return out


def compare(got, ref, tol, tol_avg):
    for k, v in ref.items():
        if isinstance(v, dict):
            for o in v:
                t = tol_avg if k.startswith("average") else tol
                assert rel(got[k][o], v[o]) < t, (k, o, rel(got[k][o], v[o]))
            continue
        t = tol_avg if k.startswith("average") or k == "com_linear_velocity" else tol
        g = np.asarray(got[k], np.float64).reshape(v.shape)
        assert rel(g, v) < t, (k, rel(g, v))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rep", REPS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_functions_equal_the_reference_definitions_gpu(models, name, rep, dtype):
    model = models(name)
    N = 37  # not a multiple of any tile
    d0 = cr.random_data(model, N, seed=11, dtype=dtype, rep=rep)
    d = helpers.upcast(d0, model) if dtype == np.float32 else d0
    got = functional(model, device_data(model, d0, rep, dtype), rep)
    ref = cr.restate(model, d, rep)
    if dtype == np.float64:
        compare(got, ref, 1e-10, 1e-10)
    else:
        compare(got, ref, FP32_TOL[name], FP32_TOL_AVG.get(name, FP32_TOL[name]))


@pytest.mark.gpu
@pytest.mark.parametrize("rep", REPS)
def test_one_environment_returns_unbatched_shapes_gpu(models, rep):
    model = models("anymal")
    d = cr.random_data(model, 1, seed=3, rep=rep)
    data = js.data.JaxSimModelData.build(
        model, base_position=d.base_position[0], base_quaternion=d.base_quaternion[0], joint_positions=d.joint_positions[0],
        joint_velocities=d.joint_velocities[0], base_linear_velocity=d.base_velocity(rep)[0, :3],
        base_angular_velocity=d.base_velocity(rep)[0, 3:], velocity_representation=_JREP[rep])  # fmt: skip
    n = model.dofs()
    assert np.shape(js.com.com_position(model, data)) == (3,)
    assert np.shape(js.com.centroidal_momentum_jacobian(model, data)) == (6, 6 + n)
    assert np.shape(js.model.kinetic_energy(model, data)) == ()
    ref = cr.restate(model, d, rep)
    assert rel(js.com.centroidal_momentum(model, data), ref["centroidal_momentum"][0]) < 1e-10
    assert rel(js.model.total_momentum_jacobian(model, data), ref["total_momentum_jacobian_out"][rep][0]) < 1e-10
    assert rel(js.model.mechanical_energy(model, data), ref["mechanical_energy"][0]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "chain5", "box"])
@pytest.mark.parametrize("rep", REPS)
def test_device_self_consistency_gpu(models, name, rep):
    """total_momentum_jacobian = free_floating_mass_matrix[:6]; 2 K = nu^T M nu with the device M."""
    model = models(name)
    d = cr.random_data(model, 9, seed=4, rep=rep)
    data = device_data(model, d, rep, np.float64)
    M = np.asarray(js.model.free_floating_mass_matrix(model, data), np.float64)
    assert rel(js.model.total_momentum_jacobian(model, data), M[:, :6]) < 1e-12
    nu = np.asarray(data.generalized_velocity, np.float64)
    assert rel(2.0 * np.asarray(js.model.kinetic_energy(model, data)), np.einsum("ni,nij,nj->n", nu, M, nu)) < 1e-12


def _data_with(model, base_position, quat, s, vB_mixed, sd):
    return js.data.JaxSimModelData.build(model, base_position=base_position, base_quaternion=quat, joint_positions=s,
                                         joint_velocities=sd, base_linear_velocity=vB_mixed[:, :3],
                                         base_angular_velocity=vB_mixed[:, 3:], velocity_representation=ja.VelRepr.Mixed)  # fmt: skip


@pytest.mark.gpu
def test_com_velocity_is_the_derivative_of_the_com_position_gpu(models):
    """Central difference of com_position along q(t) = q (+) t qdot(nu) (base pose integrated exactly for a constant
    mixed velocity over +-h) equals com_linear_velocity."""
    import maxcoord

    model = models("anymal")
    d = cr.random_data(model, 4, seed=21)
    v = d.base_velocity(VelRepr.Mixed)
    R0 = np.stack([maxcoord.quat_matrix(q) for q in d.base_quaternion])
    data = _data_with(model, d.base_position, d.base_quaternion, d.joint_positions, v, d.joint_velocities)
    vG = np.asarray(js.com.com_linear_velocity(model, data), np.float64)
    h = 1e-5

    def com_at(t):
        Rt = np.stack([_exp(w * t) for w in v[:, 3:]]) @ R0
        q = _quat(Rt)
        dd = _data_with(model, d.base_position + t * v[:, :3], q, d.joint_positions + t * d.joint_velocities, v, d.joint_velocities)
        return np.asarray(js.com.com_position(model, dd), np.float64)

    fd = (com_at(h) - com_at(-h)) / (2 * h)
    err = rel(fd, vG)
    helpers.note("centroidal_fd_com_velocity", err)
    assert err < 1e-10  # (measured 6.7e-12)


def _exp(phi):
    th = float(np.linalg.norm(phi))
    import maxcoord

    return np.eye(3) if th == 0.0 else maxcoord.axis_angle_matrix(phi / th, th)


def _quat(R):
    """Rotation matrices -> unit quaternions wxyz (Shepperd's method)."""
    out = np.zeros((R.shape[0], 4))
    for k, M in enumerate(R):
        t = np.trace(M)
        i = int(np.argmax([t, M[0, 0], M[1, 1], M[2, 2]]))
        if i == 0:
            s = 2.0 * np.sqrt(1.0 + t)
            out[k] = [0.25 * s, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s]
        elif i == 1:
            s = 2.0 * np.sqrt(1.0 + M[0, 0] - M[1, 1] - M[2, 2])
            out[k] = [(M[2, 1] - M[1, 2]) / s, 0.25 * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s]
        elif i == 2:
            s = 2.0 * np.sqrt(1.0 + M[1, 1] - M[0, 0] - M[2, 2])
            out[k] = [(M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, 0.25 * s, (M[1, 2] + M[2, 1]) / s]
        else:
            s = 2.0 * np.sqrt(1.0 + M[2, 2] - M[0, 0] - M[1, 1])
            out[k] = [(M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, 0.25 * s]
    return out


@pytest.mark.gpu
def test_free_flight_momentum_gpu(models):
    """RungeKutta4, fp64, a floating chain high in the air: the linear centroidal momentum changes by m g dt per step and
    the angular one is constant to integrator order."""
    model = free_flight_model(models)
    d = cr.random_data(model, 4, seed=31)
    d.base_position[:, 2] += 100.0  # far from the ground: no contact
    data = device_data(model, d.update_caches(model), VelRepr.Mixed, np.float64)
    m = float(model.kin_dyn_parameters.link_mass.sum())
    h0 = np.asarray(js.com.centroidal_momentum(model, data), np.float64)
    hs = [h0]
    for _ in range(FLIGHT_STEPS):
        data = js.model.step(model, data)
        hs.append(np.asarray(js.com.centroidal_momentum(model, data), np.float64))
    hs = np.stack(hs)
    dlin = np.diff(hs[:, :, :3], axis=0)
    expect = np.zeros(3)
    expect[2] = m * model.gravity * model.time_step
    lin_err = float(np.abs(dlin - expect).max()) / (m * 9.81 * model.time_step)
    ang_drift = float(np.abs(hs[:, :, 3:] - h0[None, :, 3:]).max()) / max(1.0, float(np.abs(h0[:, 3:]).max()))
    helpers.note("centroidal_free_flight_linear_per_step", lin_err)
    helpers.note("centroidal_free_flight_angular_drift", ang_drift)
    assert lin_err < 5e-11  # (measured 3.5e-12 of m g dt)
    assert ang_drift < 2e-12  # (measured 1.1e-13 over 200 steps)


@pytest.mark.gpu
def test_fixed_base_energy_drift_is_fourth_order_gpu(models):
    """K - U (the physical energy, given the reference's sign of U) of an undamped fixed-base chain under RungeKutta4:
    the drift over two seconds shrinks ~16x when the time step halves (time steps large enough for the drift to stand
    clear of the rounding: at 8 / 4 ms it is 2.4e-14 / 1.5e-15)."""
    base = fixed_chain_model(models)
    drift = {}
    for dt in (32e-3, 16e-3):
        model = helpers.with_params(base, time_step=dt)
        d = cr.random_data(model, 2, seed=41, base_velocity=False)
        d.joint_positions[:] = [[1.0, 0.5], [-0.7, 1.2]]
        d.joint_velocities[:] = [[0.0, 0.3], [0.5, -0.2]]
        data = device_data(model, d.update_caches(model), VelRepr.Mixed, np.float64)
        e0 = np.asarray(js.model.kinetic_energy(model, data)) - np.asarray(js.model.potential_energy(model, data))
        worst = 0.0
        for _ in range(int(round(2.0 / dt))):
            data = js.model.step(model, data)
            e = np.asarray(js.model.kinetic_energy(model, data)) - np.asarray(js.model.potential_energy(model, data))
            worst = max(worst, float(np.abs(e - e0).max() / np.abs(e0).max()))
        drift[dt] = worst
    helpers.note("centroidal_rk4_energy_drift_dt32ms", drift[32e-3])
    helpers.note("centroidal_rk4_energy_drift_dt16ms", drift[16e-3])
    assert drift[16e-3] < 1e-11  # (measured 1.3e-12; 3.7e-11 at 32 ms)
    assert drift[32e-3] / max(drift[16e-3], 1e-300) > 8.0, drift


@pytest.mark.gpu
def test_device_resident_extension_gpu(models):
    model = models("icub")
    d = cr.random_data(model, 70, seed=51)
    data = device_data(model, d, VelRepr.Mixed, np.float64)
    n = model.dofs()
    out = DeviceArray(24, 70, np.float64, tile=data._state.tile)
    outJ = DeviceArray(6 * (6 + n), 70, np.float64, tile=data._state.tile)
    rec, J = js.com.centroidal_quantities(model, data, jacobian=True, out=out, out_jacobian=outJ)
    assert rec is out and J is outJ
    r0, J0 = rec.to_host().copy(), J.to_host().copy()
    for _ in range(8):
        r, Jk = js.com.centroidal_quantities(model, data, jacobian=True, out=out, out_jacobian=outJ)
        assert np.array_equal(r.to_host(), r0) and np.array_equal(Jk.to_host(), J0)
    fresh = js.data.JaxSimModelData.from_state_block(model, data.state_block(), ja.VelRepr.Mixed)
    assert np.array_equal(np.asarray(js.com.com_position(model, fresh)), r0[0:3].T)
    assert np.array_equal(np.asarray(js.com.centroidal_momentum(model, fresh)), r0[3:9].T)
    assert np.array_equal(np.asarray(js.com.centroidal_momentum_jacobian(model, fresh)), J0.T.reshape(70, 6, 6 + n))
    assert np.array_equal(np.asarray(js.model.kinetic_energy(model, fresh)), r0[21])
    only = js.com.centroidal_quantities(model, data)
    assert np.array_equal(only.to_host(), r0)


@pytest.mark.gpu
def test_one_launch_serves_the_queries_of_a_state_gpu(models, monkeypatch):
    model = models("anymal")
    data = device_data(model, cr.random_data(model, 5, seed=61), VelRepr.Mixed, np.float64)
    calls = []
    real = js.com.centroidal_quantities
    monkeypatch.setattr(js.com, "centroidal_quantities", lambda *a, **k: calls.append(k) or real(*a, **k))
    js.com.com_position(model, data)
    js.com.centroidal_momentum(model, data)
    js.model.kinetic_energy(model, data)
    assert len(calls) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub"])
def test_specialised_centroidal_kernel_equals_the_library_kernel(models, name, monkeypatch):
    model = models(name)
    d = cr.random_data(model, 19, seed=71)
    block = helpers.odata_to_block(model, d)

    def run():
        data = js.data.JaxSimModelData.from_state_block(model, block, ja.VelRepr.Mixed)
        rec, J = js.com.centroidal_quantities(model, data, jacobian=True)
        return rec.to_host(), J.to_host()

    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "0")
    model.__dict__.pop("_device", None)
    ref = run()
    assert specialize.MODE_CENTROIDAL not in specialize.modes(runtime.device_model(model, np.float64))
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "require")
    model.__dict__.pop("_device", None)
    out = run()
    assert specialize.MODE_CENTROIDAL in specialize.modes(runtime.device_model(model, np.float64))
    model.__dict__.pop("_device", None)
    for x, y in zip(out, ref):
        assert helpers.rel_err(x, y) < 1e-12
