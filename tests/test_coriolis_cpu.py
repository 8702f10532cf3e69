"""Coriolis matrix (js.model.free_floating_coriolis_matrix; MODE_CORIOLIS) on the CPU.

1. The restatement of tests/coriolis_ref.py pinned without the reference, fp64, in the three representations: ``C nu``
   equals ``h - g`` of the oracle, ``Mdot - 2C`` is skew-symmetric with ``Mdot`` a central difference of the oracle's
   mass matrix along ``qdot``; its ``L_Jdot_WL_B`` equals the oracle's Inertial derivative moved to Body.
2. The kernel core of MODE_CORIOLIS (host emulation, tests/emul/jxs_emul_query.cpp) against the restatement: fp64 at
   1e-11, fp32 per-model gates; the mass matrix of the same launch against the oracle's; the host conversion of
   ``api/model.py`` to Body and Inertial.  The outputs start as NaN: an entry the kernel does not write must be a
   structural zero.
3. ``jxs_coriolis`` refuses bad arguments with JXS_EINVAL before any device call.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import query_emul
import coriolis_ref as cref
import helpers
import jaxsim_amd as ja
from coriolis_ref import TEXTS, model_of
from jaxsim_amd import _lib
from jaxsim_amd.api import model as jm
from oracle import VelRepr
from oracle import refstep as rs

# fp32: measured relative error of the emulation against the fp64 restatement (seed 3, N = 4) x 3; measured:
# anymal 6.5e-8, icub 7.2e-8, octopod 1.3e-7, cartpole 1.6e-7, chain5 1.1e-7, box 3.1e-8, lumped 1.5e-7, chain9f 1.2e-7
FP32_TOL = {"anymal": 2e-7, "icub": 2.2e-7, "octopod": 4e-7, "cartpole": 5e-7, "chain5": 3.3e-7, "box": 1e-7, "lumped": 4.5e-7,
            "chain9f": 3.6e-7}
REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


def with_rep(model, d, rep):
    out = dataclasses.replace(d, velocity_representation=rep)
    out._model = model
    return out


def pin_data(model, N, seed):
    # a fixed base at rest: the reference's h and g drop its base velocity, its C nu does not
    return cr.random_data(model, N, seed=seed, base_velocity=model.floating_base())


# ---- 1. the restatement, pinned ---------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["anymal", "octopod", "cartpole", "chain5", "lumped", "box"])
@pytest.mark.parametrize("rep", REPS)
def test_restatement_c_nu_equals_h_minus_g(name, rep):
    model = model_of(name)
    d = with_rep(model, pin_data(model, 3, seed=1), rep)
    Cm = cref.coriolis(model, d)
    nu = d.generalized_velocity(rep)
    h_g = rs.free_floating_bias_forces(model, d) - rs.free_floating_gravity_forces(model, d)
    assert rel(np.einsum("nij,nj->ni", Cm, nu), h_g) < 1e-10


@pytest.mark.parametrize("name", ["anymal", "octopod", "cartpole", "chain5", "lumped", "box"])
@pytest.mark.parametrize("rep", REPS)
def test_restatement_mdot_minus_2c_is_skew(name, rep):
    model = model_of(name)
    d = with_rep(model, pin_data(model, 3, seed=2), rep)
    Cm = cref.coriolis(model, d)
    h = 1e-5
    Md = (rs.free_floating_mass_matrix(model, with_rep(model, cref.advance(model, d, h), rep))
          - rs.free_floating_mass_matrix(model, with_rep(model, cref.advance(model, d, -h), rep))) / (2 * h)  # fmt: skip
    if not model.floating_base():
        Md[:, 0:6, 6:] = 0.0
        Md[:, 6:, 0:6] = 0.0
    assert rel(Md - Cm - np.swapaxes(Cm, -1, -2), np.zeros_like(Md)) / max(1.0, np.abs(Md).max()) < 1e-6


@pytest.mark.parametrize("name", ["anymal", "octopod", "cartpole", "lumped"])
def test_restatement_jacobian_derivative_equals_the_oracle_inertial_one_moved_to_body(name):
    model = model_of(name)
    d = cr.random_data(model, 3, seed=4)
    assert rel(cref.jacobian_derivative_body(model, d), cref.jacobian_derivative_body_via_inertial(model, d)) < 1e-12


# ---- 2. the kernel core (host emulation) ------------------------------------------------------------------------


def emulate(model, d, dtype):
    block = helpers.odata_to_block(model, d, dtype=dtype)
    Cn, Mn = query_emul.run_coriolis(model, block, dtype=dtype)  # NaN where the kernel does not write
    C0, M0 = query_emul.run_coriolis(model, block, fill=0.0, dtype=dtype)  # what jxs_coriolis hands the kernel
    np.testing.assert_array_equal(np.nan_to_num(Cn), C0)
    np.testing.assert_array_equal(np.nan_to_num(Mn), M0)
    return Cn, C0, M0


@pytest.mark.parametrize("name", list(TEXTS))
def test_kernel_core_equals_the_restatement_fp64(name):
    model = model_of(name)
    d = cr.random_data(model, 5, seed=2)  # (fixed bases: a non-zero stored base velocity)
    Cn, C0, M0 = emulate(model, d, np.float64)
    ref = cref.coriolis(model, with_rep(model, d, VelRepr.Mixed))
    assert rel(C0, ref) < 1e-11
    scale = max(1.0, np.abs(ref).max())
    assert np.all(np.abs(ref[np.isnan(Cn)]) < 1e-13 * scale)  # unwritten entries are structural zeros
    assert rel(M0, rs.free_floating_mass_matrix(model, with_rep(model, d, VelRepr.Mixed))) < 1e-12
    # the host conversion of api/model.py to Body and Inertial
    v = d.base_velocity(VelRepr.Mixed).astype(np.float64)
    for rep in (VelRepr.Body, VelRepr.Inertial):
        jrep = ja.VelRepr.Body if rep == VelRepr.Body else ja.VelRepr.Inertial
        out = jm._coriolis_mixed_to(jrep, d.base_transform.astype(np.float64), v, C0, M0)
        assert rel(out, cref.coriolis(model, with_rep(model, d, rep))) < 1e-11


@pytest.mark.parametrize("name", list(TEXTS))
def test_kernel_core_equals_the_restatement_fp32(name):
    model = model_of(name)
    d32 = cr.random_data(model, 4, seed=3, dtype=np.float32)
    _, C0, M0 = emulate(model, d32, np.float32)
    d = with_rep(model, helpers.upcast(d32, model), VelRepr.Mixed)
    assert rel(C0, cref.coriolis(model, d)) < FP32_TOL[name]
    assert rel(M0, rs.free_floating_mass_matrix(model, d)) < FP32_TOL[name]


def test_fixed_base_keeps_the_stored_base_velocity():
    """The reference's nu includes data.base_velocity for a fixed base: C changes with it."""
    model = model_of("cartpole")
    d = cr.random_data(model, 2, seed=5)
    d0 = cr.random_data(model, 2, seed=5, base_velocity=False)
    _, C1, _ = emulate(model, d, np.float64)
    _, C2, _ = emulate(model, d0, np.float64)
    assert rel(C1, C2) > 1e-3
    assert rel(C2, cref.coriolis(model, with_rep(model, d0, VelRepr.Mixed))) < 1e-11


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_jxs_coriolis_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.jxs_coriolis(p, p, None, None, 4, None) == -1  # JXS_EINVAL
    assert b"null out_C" in lib.jxs_last_error()
    assert lib.jxs_coriolis(None, p, p, None, 4, None) == -1
    assert b"null model" in lib.jxs_last_error()
    assert lib.jxs_coriolis(p, None, p, None, 4, None) == -1
    assert b"null state" in lib.jxs_last_error()
    for N in (0, -3):  # (refused before the model handle is read: a dummy pointer is never dereferenced)
        assert lib.jxs_coriolis(p, p, p, p, N, None) == -1
        assert b"N must be positive" in lib.jxs_last_error()
