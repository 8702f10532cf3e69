"""``js.model.forward_dynamics_crb`` / ``forward_dynamics`` / ``total_mass`` (MODE_FD_CRB) on the CPU.

1. The restatement of tests/fd_crb_ref.py (M and h of the oracle, J^T f from the link Jacobians, numpy.linalg.solve)
   pinned in Inertial, Body and Mixed: equal to the oracle's ABA with random joint forces and random wrenches on every
   link, and to the maximal-coordinate solver of tests/maxcoord.py (from the URDF text) on the models of
   tests/test_maxcoord_independent.py at that file's tolerance.  Models whose base link has a pose offset get no link
   wrenches in the comparison with ABA: the reference's two paths differ there (tests/fd_crb_ref.py), which a test states.
2. The kernel core of MODE_FD_CRB (host emulation, tests/emul/jxs_emul_query.cpp) against the restatement, with and
   without joint forces / link wrenches, every force representation: fp64 at 1e-10, fp32 per-model gates.
3. The output starts as NaN: every entry is finite afterwards; a fixed base returns six exact zeros.
4. ``jxs_forward_dynamics_crb`` refuses bad arguments; ``js.model.total_mass``; ``forward_dynamics`` dispatches.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import query_emul
import fd_crb_ref as fref
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import oracle
import parity_cases as pc
from coriolis_ref import TEXTS, model_of
from jaxsim_amd import _lib
from oracle import VelRepr
from oracle import refstep as rs

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)  # index = the force representation code of the kernel
# fp32: the gates are the worst relative error of the emulation against the fp64 restatement (seed 3, N = 4, the six input
# combinations below) x 3 as measured BEFORE the kernel corrected its fp32 solution with one residual step; measured then
# (MODE_FD_CRB | the emulated MODE_FD, ABA, on the same states and inputs, against the oracle's ABA):
# anymal 2.65e-6 | 1.81e-6, icub 4.98e-5 | 1.79e-5, octopod 9.81e-5 | 4.99e-5, cartpole 1.45e-6 | 1.60e-7,
# chain5 2.74e-6 | 5.04e-7, box 2.05e-7 | 2.05e-7, lumped 6.18e-6 | 2.11e-6, chain9f 6.38e-6 | 2.96e-6
# -- at most 9 x ABA on these short trees, but 80 .. 110 x on serial chains of 40 .. 64 links (5e-3 .. 1.3e-2 against
# 4e-5 .. 6e-4, profiles/query_modes_fuzz_campaign.txt): a float32 factorisation of M, whose condition number in joint
# coordinates reaches 1e6 there (numpy.linalg.solve on the reference's float32 M loses as much).  With the residual step
# (csrc/jxs_core.h fd_crb) the same cases measure
# anymal 1.27e-6, icub 1.73e-5, octopod 4.24e-5, cartpole 3.12e-7, chain5 8.07e-7, box 2.01e-7, lumped 6.52e-7, chain9f 9.32e-7
# and the worst of 323 random trees of up to 64 links 3.0e-4; the gates stay where they were.
FP32_TOL = {"anymal": 8e-6, "icub": 1.5e-4, "octopod": 2.95e-4, "cartpole": 4.4e-6, "chain5": 8.2e-6, "box": 6.2e-7, "lumped": 1.85e-5,
            "chain9f": 1.9e-5}


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


def with_rep(model, d, rep):
    out = dataclasses.replace(d, velocity_representation=rep)
    out._model = model
    return out


# ---- 1. the restatement, pinned ---------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("rep", REPS)
def test_restatement_equals_the_oracle_aba(name, rep):
    model = model_of(name)
    d = with_rep(model, cr.random_data(model, 4, seed=1), rep)
    tau, f = helpers.random_inputs(model, 4, 2, np.float64)
    if fref.link_forces_differ_from_aba(model):
        f = None
    crb = np.concatenate(fref.forward_dynamics_crb(model, d, joint_forces=tau, link_forces=f), -1)
    aba = np.concatenate(rs.forward_dynamics_aba(model, d, joint_forces=tau, link_forces=f), -1)
    assert rel(crb, aba) < 1e-10


def test_restatement_differs_from_aba_for_body_wrenches_on_a_base_offset_model():
    """What the exclusion above excludes: with a base-link offset the Jacobians place a Body / Mixed wrench where the
    cached link transforms are, ABA where its own frames are; an Inertial wrench means the same to both."""
    model = model_of("chain5")
    assert fref.link_forces_differ_from_aba(model)
    assert not any(fref.link_forces_differ_from_aba(model_of(n)) for n in TEXTS if n != "chain5")
    d0 = cr.random_data(model, 3, seed=1)
    tau, f = helpers.random_inputs(model, 3, 2, np.float64)
    for rep, same in ((VelRepr.Inertial, True), (VelRepr.Body, False), (VelRepr.Mixed, False)):
        d = with_rep(model, d0, rep)
        crb = fref.forward_dynamics_crb(model, d, joint_forces=tau, link_forces=f)[1]
        aba = rs.forward_dynamics_aba(model, d, joint_forces=tau, link_forces=f)[1]
        assert (rel(crb, aba) < 1e-10) == same


@pytest.mark.parametrize("name", list(pc.MAXCOORD_TEXTS))
def test_restatement_equals_maximal_coordinates(name):
    text, model, d, tau, f = pc.maxcoord_case(name, 4, seed=3)  # (Mixed; no wrenches on the offset-base models)
    vd, sdd = pc.maxcoord_truth(text, model, d, tau, f)
    d._model = model
    cvd, csdd = fref.forward_dynamics_crb(model, d, joint_forces=tau, link_forces=f)
    assert rel(csdd, sdd) < 1e-10
    if model.floating_base():
        assert rel(cvd, vd) < 1e-10


# ---- 2. the kernel core (host emulation) ------------------------------------------------------------------------

INPUTS = [(False, None), (True, None), (False, 0), (True, 0), (True, 1), (True, 2)]  # (joint forces?, force representation)


def emulate(model, d, dtype, tau, f, code):
    """Accelerations of the emulated launch, [N, 6+n]: inertial-fixed base acceleration, joint accelerations."""
    N = d.batch_size
    kw = {}
    if tau is not None:
        kw["tau"] = tau.T
    if f is not None:
        kw.update(link_forces=f.reshape(N, -1).T, force_repr=code)
    out = query_emul.run_fd_crb(model, helpers.odata_to_block(model, d, dtype=dtype), dtype=dtype, **kw).T
    assert np.all(np.isfinite(out))  # (the output started as NaN)
    return out


def restated(model, d64, tau, f, code):
    """The restatement in the representation the wrenches are given in; its base acceleration is compared through the
    joint accelerations and, in Inertial representation (what the kernel writes), directly."""
    rep = REPS[code if code is not None else 0]
    t64 = None if tau is None else tau.astype(np.float64)
    f64 = None if f is None else f.astype(np.float64)
    sdd = fref.forward_dynamics_crb(model, with_rep(model, d64, rep), joint_forces=t64, link_forces=f64)[1]
    W_f = None if f is None else rs.other_representation_to_inertial(f64, rep, jacobian_link_transforms(model, d64), is_force=True)
    vd = fref.forward_dynamics_crb(model, with_rep(model, d64, VelRepr.Inertial), joint_forces=t64, link_forces=W_f)[0]
    return np.concatenate([vd, sdd], -1)


def jacobian_link_transforms(model, d):
    """W_H_L as the link Jacobians see them: the cached transforms without the base-link offset of quirk 12 (the same
    as the cached ones for every model without one)."""
    H = d.link_transforms.astype(np.float64).copy()
    off = np.asarray(model.kin_dyn_parameters.suc_H_i[0][:3, 3], np.float64)
    H[:, :, :3, 3] -= np.einsum("nij,j->ni", d.base_transform[:, :3, :3].astype(np.float64), off)[:, None, :]
    return H


def worst_error(name, dtype, run=emulate):
    model = model_of(name)
    N = 4
    d = cr.random_data(model, N, seed=3, dtype=dtype)
    d64 = helpers.upcast(d, model) if dtype == np.float32 else d
    tau, f = helpers.random_inputs(model, N, 2, dtype)
    worst = 0.0
    for with_tau, code in INPUTS:
        t, w = (tau if with_tau else None), (f if code is not None else None)
        worst = max(worst, rel(run(model, d, dtype, t, w, code), restated(model, d64, t, w, code)))
    return worst


@pytest.mark.parametrize("name", list(TEXTS))
def test_kernel_core_equals_the_restatement_fp64(name):
    assert worst_error(name, np.float64) < 1e-10


@pytest.mark.parametrize("name", list(TEXTS))
def test_kernel_core_equals_the_restatement_fp32(name):
    err = worst_error(name, np.float32)
    print(f"fd_crb emulation fp32 {name}: {err:.3e}")
    assert err < FP32_TOL[name]


# ---- 3. every entry is written ----------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_entry_is_written_and_a_fixed_base_is_exactly_zero(name, dtype):
    model = model_of(name)
    d = cr.random_data(model, 5, seed=4, dtype=dtype)
    tau, f = helpers.random_inputs(model, 5, 5, dtype)
    out = query_emul.run_fd_crb(model, helpers.odata_to_block(model, d, dtype=dtype), tau=tau.T, link_forces=f.reshape(5, -1).T,
                          force_repr=2, fill=np.nan, dtype=dtype)  # fmt: skip
    assert out.shape == (6 + model.dofs(), 5) and np.all(np.isfinite(out))
    if not model.floating_base():
        assert not np.any(out[:6])


# ---- 4. the C ABI and the Python surface ------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_jxs_forward_dynamics_crb_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.jxs_forward_dynamics_crb(p, p, None, None, 0, None, 4, None) == -1  # JXS_EINVAL
    assert b"null out_acc" in lib.jxs_last_error()
    assert lib.jxs_forward_dynamics_crb(None, p, None, None, 0, p, 4, None) == -1
    assert b"null model" in lib.jxs_last_error()
    assert lib.jxs_forward_dynamics_crb(p, None, None, None, 0, p, 4, None) == -1
    assert b"null state" in lib.jxs_last_error()
    for N in (0, -3):  # (refused before the model handle is read: a dummy pointer is never dereferenced)
        assert lib.jxs_forward_dynamics_crb(p, p, None, None, 0, p, N, None) == -1
        assert b"N must be positive" in lib.jxs_last_error()
    assert "jxs_forward_dynamics_crb" in _lib.EXPORTED_SYMBOLS


def test_total_mass():
    model = model_of("anymal")
    assert js.model.total_mass(model) == model.total_mass() == float(np.sum(model.kin_dyn_parameters.link_mass))


def test_forward_dynamics_dispatches_on_prefer_aba(monkeypatch):
    calls = []
    monkeypatch.setattr(js.model, "forward_dynamics_aba", lambda model, data, **kw: calls.append(("aba", kw)) or "A")
    monkeypatch.setattr(js.model, "forward_dynamics_crb", lambda model, data, **kw: calls.append(("crb", kw)) or "C")
    assert js.model.forward_dynamics("m", "d", joint_forces=1, link_forces=2) == "A"
    assert js.model.forward_dynamics("m", "d", joint_forces=3, prefer_aba=False) == "C"
    assert calls == [("aba", dict(joint_forces=1, link_forces=2)), ("crb", dict(joint_forces=3, link_forces=None))]
