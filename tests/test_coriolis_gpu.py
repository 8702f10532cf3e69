"""Coriolis matrix on the GPU (``js.model.free_floating_coriolis_matrix``, ``js.model.coriolis_matrix_device``,
``jxs_coriolis``).

1. The public function against the reference's definition (tests/coriolis_ref.py) in Inertial, Body and Mixed, fp64 and
   fp32, N not a multiple of the tile; N = 1 returns unbatched shapes.
2. Oracle-free device checks: ``C nu = h - g`` from the existing kernels, ``Mdot - 2C`` skew-symmetric with ``Mdot`` a
   central difference of the device mass matrix, the mass matrix of the same launch equals ``jxs_mass_matrix``.
3. Library kernel against the model-specialised MODE_CORIOLIS kernel; the device-resident extension reuses its buffers.
"""
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import coriolis_ref as cref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
from jaxsim_amd import robots, runtime, specialize
from oracle import VelRepr

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)
JREPS = (ja.VelRepr.Inertial, ja.VelRepr.Body, ja.VelRepr.Mixed)
NAMES = ["anymal", "icub", "cartpole", "chain5", "box", "lumped"]
# fp32: measured worst relative error against the fp64 restatement over the three representations (N = 37, seed 11,
# library kernels, MI355X) x 3; measured: anymal 1.44e-7, icub 1.56e-7, cartpole 3.37e-7, chain5 1.42e-7, box 5.2e-8,
# lumped 1.22e-7
FP32_TOL = {"anymal": 4.5e-7, "icub": 5e-7, "cartpole": 1.1e-6, "chain5": 4.5e-7, "box": 2e-7, "lumped": 4e-7}
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_function_equals_the_reference_definition_gpu(models, name, I, dtype):
    model = model_of(models, name)
    N = 37  # not a multiple of any tile
    d0 = cr.random_data(model, N, seed=11, dtype=dtype)  # (fixed bases: a non-zero stored base velocity)
    d = with_rep(model, helpers.upcast(d0, model) if dtype == np.float32 else d0, I)
    data = device_data(model, d0, I, dtype)
    C = js.model.free_floating_coriolis_matrix(model, data)
    assert C.shape == (N, 6 + model.dofs(), 6 + model.dofs()) and C.dtype == np.dtype(dtype)
    assert rel(C, cref.coriolis(model, d)) < (1e-10 if dtype == np.float64 else FP32_TOL[name])


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
    C = js.model.free_floating_coriolis_matrix(model, data)
    assert np.shape(C) == (6 + model.dofs(), 6 + model.dofs())
    assert rel(C, cref.coriolis(model, d)[0]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub", "cartpole", "box"])
@pytest.mark.parametrize("I", [0, 1, 2])
def test_c_nu_equals_h_minus_g_gpu(models, name, I):
    model = model_of(models, name)
    d = cr.random_data(model, 9, seed=21, base_velocity=model.floating_base())  # (h, g: a fixed base at rest)
    data = device_data(model, d, I)
    C = js.model.free_floating_coriolis_matrix(model, data)
    nu = with_rep(model, d, I).generalized_velocity(REPS[I])
    h_g = np.asarray(js.model.free_floating_bias_forces(model, data)) - np.asarray(js.model.free_floating_gravity_forces(model, data))
    assert rel(np.einsum("nij,nj->ni", C, nu), h_g) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "cartpole", "lumped"])
@pytest.mark.parametrize("I", [0, 1, 2])
def test_mdot_minus_2c_is_skew_gpu(models, name, I):
    model = model_of(models, name)
    d = with_rep(model, cr.random_data(model, 5, seed=31, base_velocity=model.floating_base()), I)
    C = np.asarray(js.model.free_floating_coriolis_matrix(model, device_data(model, d, I)))
    h = 1e-5
    Mp = np.asarray(js.model.free_floating_mass_matrix(model, device_data(model, cref.advance(model, d, h), I)))
    Mm = np.asarray(js.model.free_floating_mass_matrix(model, device_data(model, cref.advance(model, d, -h), I)))
    Md = (Mp - Mm) / (2 * h)
    if not model.floating_base():
        Md[:, 0:6, 6:] = 0.0
        Md[:, 6:, 0:6] = 0.0
    assert np.abs(Md - C - np.swapaxes(C, -1, -2)).max() / max(1.0, np.abs(Md).max()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub", "chain5", "box"])
def test_mass_matrix_of_the_launch_equals_jxs_mass_matrix_gpu(models, name):
    model = model_of(models, name)
    N, nv = 13, 6 + model.dofs()
    data = device_data(model, cr.random_data(model, N, seed=41), 2)
    _, Md = js.model.coriolis_matrix_device(model, data, mass_matrix=True)
    M = Md.to_host().T.reshape(N, nv, nv)
    assert rel(M, js.model.free_floating_mass_matrix(model, data)) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["anymal", "icub"])
def test_specialised_coriolis_kernel_equals_the_library_kernel(models, name, monkeypatch):
    model = models(name)
    block = helpers.odata_to_block(model, cr.random_data(model, 19, seed=71))

    def run():
        data = js.data.JaxSimModelData.from_state_block(model, block, ja.VelRepr.Mixed)
        C, M = js.model.coriolis_matrix_device(model, data, mass_matrix=True)
        return C.to_host(), M.to_host()

    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "0")
    model.__dict__.pop("_device", None)
    ref = run()
    assert specialize.MODE_CORIOLIS not in specialize.modes(runtime.device_model(model, np.float64))
    monkeypatch.setenv("JAXSIM_AMD_SPECIALIZE", "require")
    model.__dict__.pop("_device", None)
    out = run()
    assert specialize.MODE_CORIOLIS in specialize.modes(runtime.device_model(model, np.float64))
    model.__dict__.pop("_device", None)
    for a, b in zip(out, ref):
        assert rel(a, b) < 1e-12


@pytest.mark.gpu
def test_device_resident_extension_reuses_its_buffers_gpu(models):
    model = lumped()
    N, nv = 11, 6 + model.dofs()
    d = cr.random_data(model, N, seed=9)
    data = device_data(model, d, 2)
    C, M = js.model.coriolis_matrix_device(model, data, mass_matrix=True)
    c1, m1 = C.to_host().copy(), M.to_host().copy()
    C2, M2 = js.model.coriolis_matrix_device(model, data, out=C, out_mass_matrix=M)
    assert C2 is C and M2 is M
    np.testing.assert_array_equal(C.to_host(), c1)
    np.testing.assert_array_equal(M.to_host(), m1)
    assert js.model.coriolis_matrix_device(model, data, out=C) is C
    np.testing.assert_array_equal(C.to_host(), c1)
    np.testing.assert_array_equal(c1.T.reshape(N, nv, nv), js.model.free_floating_coriolis_matrix(model, data))
    with pytest.raises(ValueError):
        js.model.coriolis_matrix_device(model, data, out=M, out_mass_matrix=runtime.DeviceArray(nv, N, np.float64, tile=data._state.tile))
