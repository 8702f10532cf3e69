"""Centroidal momentum, CoM and energies (js.com, js.model momentum / energy functions; MODE_CENTROIDAL) on the CPU.

1. The reference's definitions as restated in tests/centroidal_ref.py (oracle CRBA + cached kinematics + the
   reference's adjoints) against an independent statement from the URDF text (tests/maxcoord.py's parser: plain sums
   over the massive URDF bodies), fp64 1e-12; the sign of the reference's potential energy.
2. The kernel core of MODE_CENTROIDAL (host emulation, tests/emul/jxs_emul_query.cpp) against the restatement,
   fp64 1e-10 and fp32, on the zoo, a fixed base with a stored base velocity, a model without joints and a base 1 km
   from the origin -- with the harness's check that the mode touches no LDS and writes every output entry.
"""
import numpy as np
import pytest

import query_emul
import centroidal_ref as cr
import helpers
import jaxsim_amd as ja
import maxcoord
from jaxsim_amd import robots
from oracle import VelRepr

TEXTS = {
    "cartpole": lambda: robots.cartpole_urdf(),  # fixed base, prismatic joint
    "lumped5": lambda: robots.lumped_tree_urdf(5, seed=1, fixed_base=True),
    "box": lambda: robots.box_urdf(),  # no joints
    "chain9f": lambda: robots.chain_urdf(9, fixed_base=False, seed=2),
    "lumped7f": lambda: robots.lumped_tree_urdf(7, seed=0),
    "anymal": lambda: robots.anymal12_urdf(),
    "octopod": lambda: robots.hub_urdf(8, 2, foot_boxes=4, seed=1),
    "hub12": lambda: robots.hub_urdf(12, 1, foot_boxes=2, seed=2),
    "icub": lambda: robots.icub23_urdf(),
    "planar_biped": lambda: robots.planar_biped_urdf(),
    "double_pendulum": lambda: robots.double_pendulum_urdf(),
}
# fixed bases mounted off the world origin by a fixed joint (robots.chain_urdf base_offset): the reference's cached link
# frames -- and so its com_position -- include that offset, its dynamics do not (quirk 12)
OFFSET_TEXTS = {
    "pendulum": lambda: robots.single_pendulum_urdf(),
    "chain5": lambda: robots.chain_urdf(5, fixed_base=True, seed=1),
}
_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        text = {**TEXTS, **OFFSET_TEXTS}[name]()
        _MODELS[name] = (text, ja.JaxSimModel.build_from_model_description(text))
    return _MODELS[name]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


@pytest.mark.parametrize("name", list(TEXTS))
def test_restatement_equals_the_urdf_pin(name):
    text, model = model_of(name)
    d = cr.random_data(model, 3, seed=5)
    ref = cr.restate(model, d, VelRepr.Mixed)
    p = cr.pin(text, model, d)
    assert abs(p["m"] - float(model.kin_dyn_parameters.link_mass.sum())) < 1e-12 * p["m"]
    assert rel(ref["com_position"], p["com"]) < 1e-12
    assert rel(ref["centroidal_momentum"], p["h"]) < 1e-12
    assert rel(ref["kinetic_energy"], p["K"]) < 1e-12
    assert rel(ref["locked_centroidal_spatial_inertia"], p["locked"]) < 1e-12


@pytest.mark.parametrize("name", list(OFFSET_TEXTS))
def test_restatement_places_the_com_with_the_base_link_offset(name):
    """Quirk 12: the cached link frames (and the reference's com_position) are shifted by R_B d against the dynamics."""
    text, model = model_of(name)
    d = cr.random_data(model, 3, seed=6)
    ref = cr.restate(model, d, VelRepr.Mixed)
    p = cr.pin(text, model, d)
    off = np.einsum("nij,j->ni", d.base_transform[:, :3, :3], model.kin_dyn_parameters.suc_H_i[0][:3, 3])
    assert np.abs(off).max() > 0.1
    assert rel(ref["com_position"], p["com"] + off) < 1e-12
    assert rel(ref["kinetic_energy"], p["K"]) < 1e-12


def test_potential_energy_has_the_reference_sign():
    """``potential_energy = m z_CoM model.gravity`` with gravity = -9.81 (api/model.py:62, 2436-2453): negative above
    the ground, so the reference's mechanical_energy = K + U is not the physical energy (K - U is)."""
    text, model = model_of("anymal")
    assert model.gravity == pytest.approx(-9.81)
    d = cr.random_data(model, 4, seed=1)
    ref = cr.restate(model, d, VelRepr.Mixed)
    m = float(model.kin_dyn_parameters.link_mass.sum())
    z = cr.pin(text, model, d)["com"][:, 2]
    assert np.all(z > 0)
    np.testing.assert_allclose(ref["potential_energy"], -9.81 * m * z, rtol=1e-12)
    np.testing.assert_allclose(ref["mechanical_energy"], ref["kinetic_energy"] - 9.81 * m * z, rtol=1e-12)


def emulate(model, d, dtype):
    block = helpers.odata_to_block(model, d, dtype=dtype)
    rec, J = query_emul.run_centroidal(model, block, jacobian=True, dtype=dtype)
    assert np.all(np.isfinite(rec)) and np.all(np.isfinite(J))  # every entry written (the outputs start as NaN)
    N, n = d.base_position.shape[0], model.dofs()
    return rec.T.astype(np.float64), J.T.astype(np.float64).reshape(N, 6, 6 + n)


# fp32: the average centroidal velocity solves with I_G, whose condition number is the cart-pole's weak spot (a slender pole
# on a cart: measured 6.1e-5 at 2e-5 elsewhere)
AVG_VEL_FP32 = {"cartpole": 2e-4}


def check_record(model, d, rec, J, tol, tol_avg=None):
    ref = cr.restate(model, d, VelRepr.Mixed)
    assert rel(rec[:, 0:3], ref["com_position"]) < tol
    assert rel(rec[:, 3:9], ref["centroidal_momentum"]) < tol
    G = ref["locked_centroidal_spatial_inertia"]
    off = np.einsum("nij,j->ni", d.base_transform[:, :3, :3], model.kin_dyn_parameters.suc_H_i[0][:3, 3])
    if np.abs(off).max() == 0:
        I = rec[:, 9:15]
        IG = np.stack([I[:, [0, 1, 2]], I[:, [1, 3, 4]], I[:, [2, 4, 5]]], axis=1)
        assert rel(IG, G[:, 3:, 3:]) < tol
    assert rel(rec[:, 15:21], ref["average_centroidal_velocity"]) < (tol_avg or tol)
    assert rel(rec[:, 21], ref["kinetic_energy"]) < tol
    assert rel(rec[:, 22], ref["potential_energy"]) < tol * max(1.0, float(np.abs(d.base_position).max()))
    np.testing.assert_allclose(rec[:, 23], float(model.kin_dyn_parameters.link_mass.sum()), rtol=tol)
    assert rel(J, ref["centroidal_momentum_jacobian"]) < tol


EMUL_CASES = list(TEXTS) + list(OFFSET_TEXTS)


@pytest.mark.parametrize("name", EMUL_CASES)
def test_kernel_core_equals_the_restatement_fp64(name):
    _, model = model_of(name)
    d = cr.random_data(model, 5, seed=2)  # (fixed bases: a non-zero stored base velocity)
    rec, J = emulate(model, d, np.float64)
    check_record(model, d, rec, J, 1e-10)


@pytest.mark.parametrize("name", EMUL_CASES)
def test_kernel_core_equals_the_restatement_fp32(name):
    _, model = model_of(name)
    d32 = cr.random_data(model, 5, seed=3, dtype=np.float32)
    d = helpers.upcast(d32, model)
    rec, J = emulate(model, d32, np.float32)
    check_record(model, d, rec, J, 2e-5, AVG_VEL_FP32.get(name))


@pytest.mark.parametrize("name", ["anymal", "cartpole", "chain5"])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-5)])
def test_kernel_core_a_kilometre_from_the_origin(name, dtype, tol):
    """Frame C has its origin at the base: nothing but the CoM position itself carries the 1 km."""
    _, model = model_of(name)
    d0 = cr.random_data(model, 3, seed=4, dtype=dtype, far=True)
    d = helpers.upcast(d0, model) if dtype == np.float32 else d0
    rec, J = emulate(model, d0, dtype)
    check_record(model, d, rec, J, tol, AVG_VEL_FP32.get(name) if dtype == np.float32 else None)
    assert np.all(np.abs(rec[:, 0] - 1000.0) < 2.0)


def test_fixed_base_momentum_includes_the_stored_base_velocity():
    """nu of the reference carries the stored base velocity of a fixed base: zeroing it changes the momentum."""
    _, model = model_of("cartpole")
    d = cr.random_data(model, 2, seed=8)
    d0 = cr.random_data(model, 2, seed=8, base_velocity=False)
    r1, _ = emulate(model, d, np.float64)
    r0, _ = emulate(model, d0, np.float64)
    assert np.abs(r1[:, 3:9] - r0[:, 3:9]).max() > 1e-3
    check_record(model, d0, r0, emulate(model, d0, np.float64)[1], 1e-10)


def test_record_only_launch_leaves_the_jacobian_alone():
    _, model = model_of("anymal")
    d = cr.random_data(model, 3, seed=9)
    block = helpers.odata_to_block(model, d)
    rec, J = query_emul.run_centroidal(model, block, jacobian=False)
    assert J is None and np.all(np.isfinite(rec))


def test_the_pin_is_independent_of_product_and_oracle():
    """The URDF pin uses tests/maxcoord.py (NumPy + xml.etree) for the bodies: no table of the product's parser."""
    U = maxcoord.Urdf(TEXTS["lumped7f"]())
    assert sum(1 for r in U.links.values() if r["mass"] > 0) > model_of("lumped7f")[1].number_of_links()
