"""The four single-launch query kernels (MODE_CENTROIDAL, MODE_FRAMES, MODE_CORIOLIS, MODE_FD_CRB) on the GPU on trees
the hand-picked models of their own modules do not reach: up to 64 links, one environment per wave (G = 64, six rounds
of pointer jumping), depth 63, twelve children on one link.

1. ``js.com.centroidal_quantities`` (record and Jacobian), ``js.frame.kinematics`` (every link, and a few random frame
   targets), ``js.model.free_floating_coriolis_matrix`` and ``js.model.forward_dynamics_crb`` against their restatements
   (tests/query_modes_ref.py), fp64 and fp32, at the gates of tools/fuzz/fuzz_query_modes.py: fp64 1e-10 (FD_CRB 1e-8);
   fp32 2e-5 and, for FD_CRB, max(1e-3, 3 x r32) capped at 1e-2 with r32 the fp32 error of the reference's formulation
   on the same state, computed on the host.
2. Oracle-free on the 64-link chain in fp64: ``forward_dynamics_crb == forward_dynamics_aba`` at 1e-8, ``C nu = h - g``
   at 1e-10, eight calls of each of the four kernels bit-identical.

The host restatements are computed once per model and precision (``case``).
"""
import numpy as np
import pytest

import centroidal_ref as cr
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
import query_modes_ref as qm
from jaxsim_amd import runtime
from jaxsim_amd.api import frame as jframe
from oracle import VelRepr

JREPS = (ja.VelRepr.Inertial, ja.VelRepr.Body, ja.VelRepr.Mixed)
ZOO = ("hub12", "serial12f", "planar10f")
TREES = dict(zip(("chain64", "tree33", "hub12x5"), qm.FIXED_TREES))
NAMES = list(ZOO) + list(TREES)
# (in representation, out representation) of the frame query and the representation of the link wrenches, per model
CODES = {"hub12": (0, 1, 2), "serial12f": (1, 2, 0), "planar10f": (2, 0, 1), "chain64": (2, 1, 0), "tree33": (0, 2, 1), "hub12x5": (1, 0, 2)}
# fp32, measured on an MI355X (library and model-specialised kernels, the states of `case`), worst relative error against
# the fp64 restatements | for FD_CRB the r32 of the same state:
#   NOT MEASURED YET -- the gates below are the rule's (module docstring), no measured figure stands behind them
_TREE_MODELS, _CASES = {}, {}


def model_of(zoo, name):
    if name in ZOO:
        return zoo(name)
    if name not in _TREE_MODELS:
        _TREE_MODELS[name] = ja.JaxSimModel.build_from_model_description(qm.tree_text(TREES[name]))
    return _TREE_MODELS[name]


def gpu_models(zoo):
    """Every model this module launches (``__graft_entry__.prebuild_specialised`` builds their kernels)."""
    return [model_of(zoo, n) for n in NAMES]


def batch_of(model):
    """Five one-environment tiles for the models that take a whole wave per environment, 37 (no multiple of any tile) otherwise."""
    return 5 if model.number_of_links() > 32 else 37


def case(zoo, name, dtype):
    """State, inputs, frame targets and the float64 truths of a model and precision: computed once, never changed."""
    key = (name, np.dtype(dtype).name)
    if key not in _CASES:
        model = model_of(zoo, name)
        N = batch_of(model)
        I, O, code = CODES[name]
        d0 = cr.random_data(model, N, seed=11, dtype=dtype)  # (fixed bases: a non-zero stored base velocity)
        d64 = helpers.upcast(d0, model) if dtype == np.float32 else d0
        tau, f = helpers.random_inputs(model, N, 12, dtype)
        frames = qm.random_frames(model, np.random.default_rng(13))
        ref = qm.truths(model, d64, tau.astype(np.float64), f.astype(np.float64), code, frames, I, O)
        r32 = qm.fd_crb_fp32(model, d0, tau, f, code, ref["FDCRB"]) if dtype == np.float32 else None
        for v in (tau, f, frames[0], frames[1], ref["COR"], ref["M"], ref["FDCRB"]):
            v.setflags(write=False)
        _CASES[key] = dict(model=model, N=N, d0=d0, d64=d64, tau=tau, f=f, frames=frames, ref=ref, r32=r32, block=helpers.odata_to_block(model, d0, dtype=dtype))
    return _CASES[key]


def device_data(c, rep_code):
    return js.data.JaxSimModelData.from_state_block(c["model"], c["block"], JREPS[rep_code])


def centroidal(c):
    model, N = c["model"], c["N"]
    rec, J = js.com.centroidal_quantities(model, device_data(c, 2), jacobian=True)
    return rec.to_host().T.astype(np.float64), J.to_host().T.astype(np.float64).reshape(N, 6, 6 + model.dofs())


def frames(c, name, targets=None):
    """``(record [N, nt, 24], J [N, nt, 6, 6+n])`` of every link, or of the given ``(parent, L_H_F)`` targets."""
    model, N = c["model"], c["N"]
    I, O, _ = CODES[name]
    data = device_data(c, I)
    if targets is None:
        rec, J = js.frame.kinematics(model, data, output_vel_repr=JREPS[O], jacobian=True)
        nt = model.number_of_links()
    else:
        table = jframe.Targets(runtime.device_model(model, data.dtype), *targets)
        rec, J = jframe._launch(model, data, table, JREPS[O], True)
        nt = table.n
    return rec.to_host().T.astype(np.float64).reshape(N, nt, 24), J.to_host().T.astype(np.float64).reshape(N, nt, 6, 6 + model.dofs())


def fd_crb(c, name):
    vd, sdd = js.model.forward_dynamics_crb(c["model"], device_data(c, CODES[name][2]), joint_forces=c["tau"], link_forces=c["f"])
    return np.asarray(vd), np.asarray(sdd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_centroidal_record_and_jacobian_equal_the_restatement_gpu(models, name, dtype):
    c = case(models, name, dtype)
    rec, J = centroidal(c)
    assert np.all(np.isfinite(rec)) and np.all(np.isfinite(J))
    err = qm.centroidal_error(c["model"], c["d64"], c["ref"]["CEN"], rec, J)
    print(f"trees centroidal {name} {np.dtype(dtype).name}: {err:.3e}")
    assert err < qm.bound("CEN", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frame_kinematics_of_links_and_frames_equal_the_restatement_gpu(models, name, dtype):
    c = case(models, name, dtype)
    rec, J = frames(c, name)
    err = qm.frames_error(c["ref"]["FRM_links"], rec, J)
    rec, J = frames(c, name, c["frames"])
    err = max(err, qm.frames_error(c["ref"]["FRM_frames"], rec, J))
    print(f"trees frames {name} {np.dtype(dtype).name}: {err:.3e}")
    assert err < qm.bound("FRM", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_coriolis_matrix_equals_the_restatement_gpu(models, name, dtype):
    c = case(models, name, dtype)
    model = c["model"]
    C = js.model.free_floating_coriolis_matrix(model, device_data(c, 2))
    nv = 6 + model.dofs()
    assert C.shape == (c["N"], nv, nv) and C.dtype == np.dtype(dtype)
    err = qm.rel(C, c["ref"]["COR"])
    print(f"trees coriolis {name} {np.dtype(dtype).name}: {err:.3e}")
    assert err < qm.bound("COR", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_forward_dynamics_crb_equals_the_restatement_gpu(models, name, dtype):
    c = case(models, name, dtype)
    model, I = c["model"], CODES[name][2]
    vd, sdd = fd_crb(c, name)
    assert vd.shape == (c["N"], 6) and sdd.shape == (c["N"], model.dofs()) and vd.dtype == sdd.dtype == np.dtype(dtype)
    # the function returns the base acceleration in the data's representation: compared through the joint accelerations and, in
    # that representation, against the restatement of it (tests/test_fd_crb_gpu.py)
    rvd, rsdd = qm.fref.forward_dynamics_crb(model, qm.with_rep(model, c["d64"], qm.REPS[I]), joint_forces=c["tau"].astype(np.float64),
                                             link_forces=c["f"].astype(np.float64))  # fmt: skip
    assert qm.rel(rsdd, c["ref"]["FDCRB"][:, 6:]) < 1e-12  # (the same restatement as the emulation campaign's)
    err = qm.rel(np.concatenate([vd, sdd], -1), np.concatenate([rvd, rsdd], -1))
    print(f"trees fd_crb {name} {np.dtype(dtype).name}: {err:.3e} (r32 {c['r32']})")
    assert err < qm.bound("FDCRB", dtype, c["r32"])
    if not model.floating_base():
        assert not np.any(vd)  # exactly zero


@pytest.mark.gpu
def test_crb_equals_aba_on_the_64_link_chain_gpu(models):
    """Oracle-free, depth 63: composite inertias + RNEA bias + the L^T D L factor of M against the articulated-body recursion."""
    c = case(models, "chain64", np.float64)
    data = device_data(c, 2)
    crb = np.concatenate(js.model.forward_dynamics_crb(c["model"], data, joint_forces=c["tau"], link_forces=c["f"]), -1)
    aba = np.concatenate(js.model.forward_dynamics_aba(c["model"], data, joint_forces=c["tau"], link_forces=c["f"]), -1)
    assert qm.rel(crb, aba) < 1e-8


@pytest.mark.gpu
def test_c_nu_equals_h_minus_g_on_the_64_link_chain_gpu(models):
    c = case(models, "chain64", np.float64)
    model = c["model"]
    data = device_data(c, 2)
    C = js.model.free_floating_coriolis_matrix(model, data)
    nu = qm.with_rep(model, c["d64"], VelRepr.Mixed).generalized_velocity(VelRepr.Mixed)
    h_g = np.asarray(js.model.free_floating_bias_forces(model, data)) - np.asarray(js.model.free_floating_gravity_forces(model, data))
    assert qm.rel(np.einsum("nij,nj->ni", C, nu), h_g) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eight_calls_are_bit_identical_on_the_64_link_chain_gpu(models, dtype):
    """One environment per wave (G = 64) was in the determinism sweep of none of the four kernels."""
    c = case(models, "chain64", dtype)
    model = c["model"]

    def all_four():
        C = js.model.free_floating_coriolis_matrix(model, device_data(c, 2))
        return centroidal(c) + frames(c, "chain64") + (np.asarray(C),) + fd_crb(c, "chain64")

    first = all_four()
    assert all(np.all(np.isfinite(a)) for a in first)
    for _ in range(7):
        for a, b in zip(all_four(), first):
            np.testing.assert_array_equal(a, b)
