"""Frames on the GPU (``js.link``, ``js.frame``, ``js.model.link_bias_accelerations``, ``js.com.bias_acceleration``,
``jxs_frame_kinematics``).

1. Every new function against the reference's definitions (tests/frames_ref.py) in the three representations and every
   ``output_vel_repr``, fp64 and fp32, N not a multiple of the tile; N = 1 returns unbatched shapes.
2. Device cross-checks against existing paths: the Jacobian kernel, the cached kinematics, ``J nu``,
   ``jacobian_derivative @ nu`` for all nine pairs, the Inertial <-> Body identity of the bias accelerations.
3. Oracle-free: finite differences in time of the link / frame velocities and of the CoM velocity.
4. The device-resident extension ``js.frame.kinematics``; one launch serves several queries of a state.
5. Library kernel against the model-specialised MODE_FRAMES kernel.
6. C ABI: refused tables, create / destroy without leaks.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import frames_ref as fr
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
from jaxsim_amd import _lib, robots, runtime, specialize
from oracle import VelRepr

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)
JREPS = (ja.VelRepr.Inertial, ja.VelRepr.Body, ja.VelRepr.Mixed)
NAMES = ["anymal", "icub", "cartpole", "chain5", "lumped"]
FP32_TOL = 2e-5
_LUMPED = []


def lumped(zoo=None):
    if not _LUMPED:
        _LUMPED.append(ja.JaxSimModel.build_from_model_description(robots.lumped_tree_urdf(5, seed=1)))
    return _LUMPED[0]


def model_of(models, name):
    return lumped() if name == "lumped" else models(name)


def gpu_models(zoo):
    """Every model this module launches (``__graft_entry__.prebuild_specialised`` builds their kernels)."""
    return [zoo(n) for n in NAMES if n != "lumped"] + [lumped()]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


def device_data(model, d, I, dtype):
    return js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d, dtype=dtype), JREPS[I])


def with_rep(model, d, I):
    out = dataclasses.replace(d, velocity_representation=REPS[I])
    out._model = model
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_functions_equal_the_reference_definitions_gpu(models, name, I, dtype):
    model = model_of(models, name)
    N = 37  # not a multiple of any tile
    d0 = cr.random_data(model, N, seed=11, dtype=dtype)
    d = with_rep(model, helpers.upcast(d0, model) if dtype == np.float32 else d0, I)
    data = device_data(model, d0, I, dtype)
    tol = 1e-10 if dtype == np.float64 else FP32_TOL
    nL = model.number_of_links()
    P, H = fr.link_targets(model)
    for O in range(3):
        ref = fr.restate(model, d, P, H, I, O)
        for L in range(nL):
            assert rel(js.link.transform(model, data, link_index=L), ref["H"][:, L]) < tol
            assert rel(js.link.bias_acceleration(model, data, link_index=L, output_vel_repr=JREPS[O]), ref["a"][:, L]) < tol
            if O != 0 or not model.kin_dyn_parameters.suc_H_i[0][:3, 3].any():  # (the link Jacobian of a base-link offset: below)
                assert rel(js.link.velocity(model, data, link_index=L, output_vel_repr=JREPS[O]), ref["v"][:, L]) < tol
                assert rel(js.link.jacobian(model, data, link_index=L, output_vel_repr=JREPS[O]), ref["J"][:, L]) < tol
        if O == I:
            assert rel(js.model.link_bias_accelerations(model, data), ref["a"]) < tol
    if model.frame_names():
        Pf, Hf = fr.frame_targets(model)
        for O in range(3):
            ref = fr.restate(model, d, Pf, Hf, I, O)
            for f in range(len(Pf)):
                fi = nL + f
                assert rel(js.frame.transform(model, data, frame_index=fi), ref["H"][:, f]) < tol
                assert rel(js.frame.velocity(model, data, frame_index=fi, output_vel_repr=JREPS[O]), ref["v"][:, f]) < tol
                assert rel(js.frame.jacobian(model, data, frame_index=fi, output_vel_repr=JREPS[O]), ref["J"][:, f]) < tol
                assert rel(js.frame.bias_acceleration(model, data, frame_index=fi, output_vel_repr=JREPS[O]), ref["a"][:, f]) < tol


@pytest.mark.gpu
@pytest.mark.parametrize("I", [0, 1, 2])
def test_one_environment_returns_unbatched_shapes_gpu(models, I):
    model = lumped()
    d = with_rep(model, cr.random_data(model, 1, seed=3), I)
    vB = d.base_velocity(REPS[I])[0]
    data = js.data.JaxSimModelData.build(
        model, base_position=d.base_position[0], base_quaternion=d.base_quaternion[0], joint_positions=d.joint_positions[0],
        joint_velocities=d.joint_velocities[0], base_linear_velocity=vB[:3], base_angular_velocity=vB[3:],
        velocity_representation=JREPS[I])  # fmt: skip
    n, nL = model.dofs(), model.number_of_links()
    assert np.shape(js.link.transform(model, data, link_index=1)) == (4, 4)
    assert np.shape(js.link.jacobian(model, data, link_index=1)) == (6, 6 + n)
    assert np.shape(js.frame.velocity(model, data, frame_index=nL)) == (6,)
    assert np.shape(js.model.link_bias_accelerations(model, data)) == (nL, 6)
    assert np.shape(js.com.bias_acceleration(model, data)) == (3,)
    ref = fr.restate(model, d, *fr.link_targets(model), I, I)
    assert rel(js.model.link_bias_accelerations(model, data), ref["a"][0]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub", "chain5"])
@pytest.mark.parametrize("I", [0, 1, 2])
def test_device_cross_checks_gpu(models, name, I):
    """Against the Jacobian kernel (MODE_JAC), the cached kinematics (MODE_KIN) and J nu."""
    model = models(name)
    data = device_data(model, cr.random_data(model, 9, seed=4), I, np.float64)
    nu = np.asarray(data.generalized_velocity, np.float64)
    Hc = np.asarray(data._link_transforms, np.float64)
    for O in range(3):
        Jall = np.asarray(js.model.generalized_free_floating_jacobian(model, data, output_vel_repr=JREPS[O]), np.float64)
        for L in range(model.number_of_links()):
            J = js.link.jacobian(model, data, link_index=L, output_vel_repr=JREPS[O])
            assert rel(J, Jall[:, L]) < 1e-12
            assert rel(js.link.velocity(model, data, link_index=L, output_vel_repr=JREPS[O]), np.einsum("nij,nj->ni", J, nu)) < 1e-12
            assert rel(js.link.transform(model, data, link_index=L), Hc[:, L]) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub"])
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("O", [0, 1, 2])
def test_bias_equals_jacobian_derivative_times_nu_gpu(models, name, I, O):
    model = models(name)
    data = device_data(model, cr.random_data(model, 7, seed=5), I, np.float64)
    nu = np.asarray(data.generalized_velocity, np.float64)
    for L in range(model.number_of_links()):
        Jd = js.link.jacobian_derivative(model, data, link_index=L, output_vel_repr=JREPS[O])
        assert rel(js.link.bias_acceleration(model, data, link_index=L, output_vel_repr=JREPS[O]), np.einsum("nij,nj->ni", Jd, nu)) < 1e-10


@pytest.mark.gpu
def test_frame_bias_equals_frame_jacobian_derivative_times_nu_gpu(models):
    model = lumped()
    nL = model.number_of_links()
    for I in range(3):
        data = device_data(model, cr.random_data(model, 5, seed=6), I, np.float64)
        nu = np.asarray(data.generalized_velocity, np.float64)
        for O in range(3):
            for f in range(len(model.frame_names())):
                Jd = js.frame.jacobian_derivative(model, data, frame_index=nL + f, output_vel_repr=JREPS[O])
                a = js.frame.bias_acceleration(model, data, frame_index=nL + f, output_vel_repr=JREPS[O])
                assert rel(a, np.einsum("nij,nj->ni", Jd, nu)) < 1e-10


@pytest.mark.gpu
def test_inertial_body_identity_of_the_bias_gpu(models):
    """The reference's conversion: W_a = W_X_L L_a for the same input representation (no cross term)."""
    model = models("anymal")
    data = device_data(model, cr.random_data(model, 6, seed=7), 2, np.float64)
    from jaxsim_amd.api.model import _adjoint

    for L in range(model.number_of_links()):
        W_a = js.link.bias_acceleration(model, data, link_index=L, output_vel_repr=ja.VelRepr.Inertial)
        L_a = js.link.bias_acceleration(model, data, link_index=L, output_vel_repr=ja.VelRepr.Body)
        W_H_L = np.asarray(js.link.transform(model, data, link_index=L), np.float64)
        assert rel(W_a, np.einsum("nij,nj->ni", _adjoint(W_H_L), L_a)) < 1e-12


def _advance_mixed(model, d, h):
    """The state after time h at constant mixed generalized velocity."""
    return fr.advance(model, with_rep(model, d, 2), 2, h)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["links", "frames"])
def test_finite_difference_in_time_gpu(models, which):
    """Oracle-free: (v(t+h) - v(t-h)) / 2h at constant Mixed nu equals the bias acceleration, on the device."""
    model = lumped() if which == "frames" else models("anymal")
    d = cr.random_data(model, 4, seed=8)
    h = 1e-5
    nL = model.number_of_links()
    idx = range(nL) if which == "links" else range(nL, nL + len(model.frame_names()))
    fn_v = (lambda m, x, i: js.link.velocity(m, x, link_index=i)) if which == "links" else (lambda m, x, i: js.frame.velocity(m, x, frame_index=i))
    fn_a = (lambda m, x, i: js.link.bias_acceleration(m, x, link_index=i)) if which == "links" else (lambda m, x, i: js.frame.bias_acceleration(m, x, frame_index=i))
    dp, dm_, d0 = (device_data(model, _advance_mixed(model, d, s), 2, np.float64) for s in (h, -h, 0.0))
    for i in idx:
        fd = (np.asarray(fn_v(model, dp, i), np.float64) - np.asarray(fn_v(model, dm_, i), np.float64)) / (2 * h)
        assert rel(fd, fn_a(model, d0, i)) < 1e-6
    if which == "frames":
        return
    # the CoM: d/dt com_linear_velocity at constant nu
    fd = (np.asarray(js.com.com_linear_velocity(model, dp)) - np.asarray(js.com.com_linear_velocity(model, dm_))) / (2 * h)
    assert rel(fd, js.com.bias_acceleration(model, d0)) < 1e-6


@pytest.mark.gpu
def test_device_resident_extension_gpu(models):
    model = lumped()
    N = 11
    d = cr.random_data(model, N, seed=9)
    data = device_data(model, d, 2, np.float64)
    rec, J = js.frame.kinematics(model, data, frame_names=model.frame_names(), jacobian=True)
    r1, J1 = rec.to_host().copy(), J.to_host().copy()
    rec2, J2 = js.frame.kinematics(model, data, frame_names=model.frame_names(), jacobian=True, out=rec, out_jacobian=J)
    assert rec2 is rec and J2 is J
    np.testing.assert_array_equal(rec.to_host(), r1)
    np.testing.assert_array_equal(J.to_host(), J1)
    fresh = device_data(model, d, 2, np.float64)
    nL, nt, n = model.number_of_links(), len(model.frame_names()), model.dofs()
    r = r1.T.reshape(N, nt, 24)
    Jh = J1.T.reshape(N, nt, 6, 6 + n)
    for f in range(nt):
        np.testing.assert_array_equal(r[:, f, 12:18], js.frame.velocity(model, fresh, frame_index=nL + f))
        np.testing.assert_array_equal(Jh[:, f], js.frame.jacobian(model, fresh, frame_index=nL + f))
    links = js.frame.kinematics(model, data).to_host().T.reshape(N, nL, 24)
    np.testing.assert_array_equal(links[..., 18:], js.model.link_bias_accelerations(model, fresh))


@pytest.mark.gpu
def test_one_launch_serves_the_queries_of_a_state_gpu(models, monkeypatch):
    model = models("anymal")
    data = device_data(model, cr.random_data(model, 5, seed=61), 2, np.float64)
    calls = []
    import jaxsim_amd.api.frame as jf

    real = jf._launch
    monkeypatch.setattr(jf, "_launch", lambda *a, **k: calls.append(1) or real(*a, **k))
    js.link.transform(model, data, link_index=2)
    js.link.velocity(model, data, link_index=3)
    js.link.bias_acceleration(model, data, link_index=4)
    js.model.link_bias_accelerations(model, data)
    assert len(calls) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub"])
def test_specialised_frames_kernel_equals_the_library_kernel(models, name, monkeypatch):
    model = models(name)
    block = helpers.odata_to_block(model, cr.random_data(model, 19, seed=71))

    def run():
        data = js.data.JaxSimModelData.from_state_block(model, block, ja.VelRepr.Mixed)
        rec, J = js.frame.kinematics(model, data, jacobian=True)
        return rec.to_host(), J.to_host()

    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "0")
    model.__dict__.pop("_device", None)
    ref = run()
    assert specialize.MODE_FRAMES not in specialize.modes(runtime.device_model(model, np.float64))
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "require")
    model.__dict__.pop("_device", None)
    out = run()
    assert specialize.MODE_FRAMES in specialize.modes(runtime.device_model(model, np.float64))
    model.__dict__.pop("_device", None)
    for a, b in zip(out, ref):
        assert rel(a, b) < 1e-12


@pytest.mark.gpu
def test_c_abi_refuses_bad_tables_and_does_not_leak(models):
    model = models("anymal")
    dm = runtime.device_model(model, np.float64)
    lib = _lib.load()
    nL = model.number_of_links()
    h = C.c_void_p()
    H = np.ascontiguousarray(np.broadcast_to(np.eye(4), (2, 4, 4)), dtype=np.float64)
    dptr = H.ctypes.data_as(C.POINTER(C.c_double))
    bad = np.array([0, nL], dtype=np.int32)
    assert lib.jxs_frames_create(dm.handle, 2, bad.ctypes.data_as(C.POINTER(C.c_int32)), dptr, C.byref(h)) == -1  # JXS_EINVAL
    assert b"parent link" in lib.jxs_last_error()
    good = np.array([0, 1], dtype=np.int32)
    gptr = good.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.jxs_frames_create(dm.handle, 0, gptr, dptr, C.byref(h)) == -1
    assert b"number of frame targets" in lib.jxs_last_error()
    H2 = H.copy()
    H2[1, 3, 0] = 0.5
    assert lib.jxs_frames_create(dm.handle, 2, gptr, H2.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)) == -1
    assert b"last row" in lib.jxs_last_error()

    def free_bytes():
        runtime.synchronize()
        free, total = C.c_size_t(), C.c_size_t()
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    many = np.arange(nL, dtype=np.int32)
    Hm = np.ascontiguousarray(np.broadcast_to(np.eye(4), (nL, 4, 4)), dtype=np.float64)
    before = free_bytes()
    for _ in range(100):
        assert lib.jxs_frames_create(dm.handle, nL, many.ctypes.data_as(C.POINTER(C.c_int32)), Hm.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)) == 0
        assert lib.jxs_frames_destroy(h) == 0
    assert free_bytes() >= before - (2 << 20)
