"""``js.model.forward_dynamics_crb`` on the GPU (``jxs_forward_dynamics_crb``, MODE_FD_CRB).

1. The public function against the restatement of the reference's CRB path (tests/fd_crb_ref.py) in Inertial, Body and
   Mixed, fp64 and fp32, random joint forces and random wrenches on every link, N not a multiple of the tile; N = 1
   returns unbatched shapes.
2. Oracle-free device checks: ``forward_dynamics_crb == forward_dynamics_aba`` (two structurally different algorithms:
   composite inertias + RNEA bias + the L^T D L factor of M against the articulated-body recursion), and
   ``inverse_dynamics`` fed with the CRB accelerations returns the joint forces and the wrench on the base link.  Models
   whose base link has a pose offset get no link wrenches there: the reference's two paths differ for them
   (tests/fd_crb_ref.py); check 1 covers those models with wrenches.
3. Library kernel against the model-specialised MODE_FD_CRB kernel; eight calls on one state are bit-identical.
"""
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import fd_crb_ref as fref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
from jaxsim_amd import robots, runtime, specialize
from oracle import VelRepr

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)
JREPS = (ja.VelRepr.Inertial, ja.VelRepr.Body, ja.VelRepr.Mixed)
NAMES = ["anymal", "icub", "cartpole", "chain5", "box", "lumped"]
# fp32: measured worst relative error against the fp64 restatement over the three representations (N = 37, seed 11,
# MI355X, library and specialised kernels) x 3; measured: anymal 2.17e-6, icub 2.14e-5, cartpole 1.44e-6, chain5 3.27e-6,
# box 2.58e-7, lumped 2.79e-6
FP32_TOL = {"anymal": 6.5e-6, "icub": 6.4e-5, "cartpole": 4.3e-6, "chain5": 9.8e-6, "box": 7.7e-7, "lumped": 8.3e-6}
_LUMPED = []


def lumped():
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


def device_data(model, d, I, dtype=np.float64):
    return js.data.JaxSimModelData.from_state_block(model, helpers.odata_to_block(model, d, dtype=dtype), JREPS[I])


def with_rep(model, d, I):
    out = dataclasses.replace(d, velocity_representation=REPS[I])
    out._model = model
    return out


def case(model, N, seed, dtype=np.float64):
    d0 = cr.random_data(model, N, seed=seed, dtype=dtype)  # (fixed bases: a non-zero stored base velocity, which h drops)
    tau, f = helpers.random_inputs(model, N, seed + 1, dtype)
    return d0, tau, f


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_function_equals_the_restatement_gpu(models, name, I, dtype):
    model = model_of(models, name)
    N = 37  # not a multiple of any tile
    d0, tau, f = case(model, N, 11, dtype)
    d = with_rep(model, helpers.upcast(d0, model) if dtype == np.float32 else d0, I)
    vd, sdd = js.model.forward_dynamics_crb(model, device_data(model, d0, I, dtype), joint_forces=tau, link_forces=f)
    assert vd.shape == (N, 6) and sdd.shape == (N, model.dofs()) and vd.dtype == sdd.dtype == np.dtype(dtype)
    rvd, rsdd = fref.forward_dynamics_crb(model, d, joint_forces=tau.astype(np.float64), link_forces=f.astype(np.float64))
    err = rel(np.concatenate([vd, sdd], -1), np.concatenate([rvd, rsdd], -1))
    print(f"fd_crb {name} rep {I} {np.dtype(dtype).name}: rel err {err:.3e}")
    assert err < (1e-10 if dtype == np.float64 else FP32_TOL[name])
    if not model.floating_base():
        assert not np.any(np.asarray(vd))  # exactly zero


@pytest.mark.gpu
@pytest.mark.parametrize("I", [0, 1, 2])
def test_one_environment_returns_unbatched_shapes_gpu(models, I):
    model = lumped()
    d0, tau, f = case(model, 1, 3)
    d = with_rep(model, d0, I)
    vB = d.base_velocity(REPS[I])[0]
    data = js.data.JaxSimModelData.build(
        model, base_position=d.base_position[0], base_quaternion=d.base_quaternion[0], joint_positions=d.joint_positions[0],
        joint_velocities=d.joint_velocities[0], base_linear_velocity=vB[:3], base_angular_velocity=vB[3:],
        velocity_representation=JREPS[I])  # fmt: skip
    vd, sdd = js.model.forward_dynamics_crb(model, data, joint_forces=tau[0], link_forces=f[0])
    assert np.shape(vd) == (6,) and np.shape(sdd) == (model.dofs(),)
    rvd, rsdd = fref.forward_dynamics_crb(model, d, joint_forces=tau, link_forces=f)
    assert rel(vd, rvd[0]) < 1e-10 and rel(sdd, rsdd[0]) < 1e-10
    # the dispatcher of the reference
    a = js.model.forward_dynamics(model, data, joint_forces=tau[0], link_forces=f[0], prefer_aba=False)
    np.testing.assert_array_equal(a[0], vd)
    np.testing.assert_array_equal(a[1], sdd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [0, 1, 2])
def test_crb_equals_aba_on_the_device_gpu(models, name, I):
    model = model_of(models, name)
    N = 37
    d0, tau, f = case(model, N, 21)
    f = None if fref.link_forces_differ_from_aba(model) else f  # (the one stated exclusion: the module docstring)
    data = device_data(model, d0, I)
    crb = np.concatenate(js.model.forward_dynamics_crb(model, data, joint_forces=tau, link_forces=f), -1)
    aba = np.concatenate(js.model.forward_dynamics_aba(model, data, joint_forces=tau, link_forces=f), -1)
    assert rel(crb, aba) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [0, 1, 2])
def test_inverse_dynamics_of_the_crb_accelerations_returns_the_forces_gpu(models, name, I):
    """The round trip of the reference's notebook: nu_dot = FD(tau, f); ID(nu_dot, f without the base wrench) = (f_0, tau)."""
    model = model_of(models, name)
    N = 9
    d0, tau, f = case(model, N, 31)
    if not model.floating_base():  # (inverse dynamics keeps the base of a fixed-base model at rest, like h)
        d0 = cr.random_data(model, N, seed=31, base_velocity=False)
    f = np.zeros_like(f) if fref.link_forces_differ_from_aba(model) else f
    data = device_data(model, d0, I)
    vd, sdd = js.model.forward_dynamics_crb(model, data, joint_forces=tau, link_forces=f)
    f_rest = f.copy()
    f_rest[:, 0] = 0.0
    fB, tq = js.model.inverse_dynamics(model, data, joint_accelerations=sdd, base_acceleration=vd, link_forces=f_rest)
    assert rel(tq, tau) < 1e-9
    if model.floating_base():
        assert rel(fB, f[:, 0]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub"])
def test_specialised_fd_crb_kernel_equals_the_library_kernel(models, name, monkeypatch):
    model = models(name)
    d0, tau, f = case(model, 19, 71)
    block = helpers.odata_to_block(model, d0)

    def run():
        data = js.data.JaxSimModelData.from_state_block(model, block, ja.VelRepr.Mixed)
        return np.concatenate(js.model.forward_dynamics_crb(model, data, joint_forces=tau, link_forces=f), -1)

    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "0")
    model.__dict__.pop("_device", None)
    ref = run()
    assert specialize.MODE_FD_CRB not in specialize.modes(runtime.device_model(model, np.float64))
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "require")
    model.__dict__.pop("_device", None)
    out = run()
    assert specialize.MODE_FD_CRB in specialize.modes(runtime.device_model(model, np.float64))
    model.__dict__.pop("_device", None)
    assert rel(out, ref) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["icub", "chain5"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eight_calls_are_bit_identical_gpu(models, name, dtype):
    model = model_of(models, name)
    d0, tau, f = case(model, 37, 81, dtype)
    data = device_data(model, d0, 2, dtype)
    first = np.concatenate(js.model.forward_dynamics_crb(model, data, joint_forces=tau, link_forces=f), -1)
    assert np.all(np.isfinite(first))
    for _ in range(7):
        again = np.concatenate(js.model.forward_dynamics_crb(model, data, joint_forces=tau, link_forces=f), -1)
        np.testing.assert_array_equal(again, first)
