"""Frames (js.link, js.frame, js.joint; js.model.link_bias_accelerations; MODE_FRAMES) on the CPU.

1. The restatement of tests/frames_ref.py pinned without the product: a central finite difference in time of
   ``O_v_WF(q(t))`` at constant ``I_nu`` (closed-form base motion for each representation) equals its ``O_Jdot_WF_I I_nu``.
2. The kernel core of MODE_FRAMES (host emulation, tests/emul/jxs_emul_query.cpp) against the restatement for all nine
   (input, output) representation pairs, with and without the Jacobian, fp64 1e-10 and fp32 per-model gates; links and
   model frames; a fixed base with a stored base velocity, a base-link offset, a base a kilometre from the origin.  The
   outputs start as NaN, so an entry the kernel does not write fails.
3. Host logic: the name / index maps, ``idx_of_parent_link``, the ValueErrors, ``js.joint.position_limits``.
"""
import dataclasses

import numpy as np
import pytest

import centroidal_ref as cr
import query_emul
import frames_ref as fr
import helpers
import jaxsim_amd as ja
import jaxsim_amd.api as js
from jaxsim_amd import robots

TEXTS = {
    "icub": lambda: robots.icub23_urdf(),
    "anymal": lambda: robots.anymal12_urdf(),
    "octopod": lambda: robots.hub_urdf(8, 2, foot_boxes=4, seed=1),
    "cartpole": lambda: robots.cartpole_urdf(),  # fixed base (stored base velocity), 2 frames
    "lumped": lambda: robots.lumped_tree_urdf(5, seed=1),  # rotated frames
    "chain5": lambda: robots.chain_urdf(5, fixed_base=True, seed=1),  # fixed base mounted with a base-link offset
    "chain9f": lambda: robots.chain_urdf(9, fixed_base=False, seed=2),
}
# fp32: worst measured relative error of the emulation over the nine pairs, x ~3
FP32_TOL = {"icub": 3e-6, "anymal": 3e-6, "octopod": 3e-6, "cartpole": 3e-6, "lumped": 3e-6, "chain5": 3e-6, "chain9f": 3e-6}
_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = ja.JaxSimModel.build_from_model_description(TEXTS[name]())
    return _MODELS[name]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max())) if ref.size else 0.0


def with_rep(model, d, I):
    out = dataclasses.replace(d, velocity_representation=fr.REPS[I])
    out._model = model
    return out


def targets(model, which):
    return fr.link_targets(model) if which == "links" else fr.frame_targets(model)


def check(model, d, d_ref, which, I, O, tol, jacobian=True, dtype=np.float64):
    P, H = targets(model, which)
    block = helpers.odata_to_block(model, d, dtype=dtype)
    rec, J = query_emul.run_frames(model, block, P, H, I, O, jacobian=jacobian, dtype=dtype)
    assert np.all(np.isfinite(rec)) and (J is None or np.all(np.isfinite(J)))  # every entry written
    ref = fr.restate(model, with_rep(model, d_ref, I), P, H, I, O)
    Hk = np.zeros(ref["H"].shape)
    Hk[..., :3, :] = rec[..., :12].reshape(rec.shape[:2] + (3, 4))
    Hk[..., 3, 3] = 1.0
    errs = dict(H=rel(Hk, ref["H"]), v=rel(rec[..., 12:18], ref["v"]), a=rel(rec[..., 18:24], ref["a"]))
    if jacobian:
        errs["J"] = rel(J, ref["J"])
    assert max(errs.values()) < tol, errs
    return max(errs.values())


def cases():
    out = []
    for name in TEXTS:
        for which in ("links", "frames"):
            if which == "frames" and len(model_of(name).frame_names()) == 0:
                continue
            out.append((name, which))
    return out


@pytest.mark.parametrize("name,which", cases())
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("O", [0, 1, 2])
def test_kernel_core_equals_the_restatement_fp64(name, which, I, O):
    model = model_of(name)
    d = cr.random_data(model, 5, seed=2)  # (fixed bases: a non-zero stored base velocity)
    check(model, d, d, which, I, O, 1e-10, jacobian=(I + O) % 2 == 0)


@pytest.mark.parametrize("name,which", cases())
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("O", [0, 1, 2])
def test_kernel_core_equals_the_restatement_fp32(name, which, I, O):
    model = model_of(name)
    d32 = cr.random_data(model, 5, seed=3, dtype=np.float32)
    check(model, d32, helpers.upcast(d32, model), which, I, O, FP32_TOL[name], jacobian=(I + O) % 2 == 1, dtype=np.float32)


@pytest.mark.parametrize("name", ["anymal", "cartpole", "chain5"])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-3)])
def test_kernel_core_a_kilometre_from_the_origin(name, dtype, tol):
    """Frame C has its origin at the base: only the Inertial outputs and the pose carry the kilometre.  (An Inertial INPUT
    in fp32 is not checked here: its base linear velocity v_W = pdot - w x p is itself the difference of kilometre-sized
    terms, a property of the representation, not of the kernel.  The state stores that inertial-fixed velocity, so in fp32
    the base's own velocity pdot = v_W + w x p carries an absolute error of ~1e3 ulp: measured 1.7e-4 in the bias rows.)"""
    model = model_of(name)
    d0 = cr.random_data(model, 3, seed=4, dtype=dtype, far=True)
    d = helpers.upcast(d0, model) if dtype == np.float32 else d0
    for I, O in ((0, 0), (1, 1), (2, 2), (2, 1), (1, 0)) if dtype == np.float64 else ((1, 1), (2, 2), (2, 1), (1, 0)):
        check(model, d0, d, "links", I, O, tol, dtype=dtype)


def test_fixed_base_bias_includes_the_stored_base_velocity():
    """The reference's link_bias_accelerations read data.base_velocity for a fixed base too."""
    model = model_of("cartpole")
    d1 = cr.random_data(model, 2, seed=8)
    d0 = cr.random_data(model, 2, seed=8, base_velocity=False)
    P, H = fr.link_targets(model)
    r1, _ = query_emul.run_frames(model, helpers.odata_to_block(model, d1), P, H, 2, 2, jacobian=False)
    r0, _ = query_emul.run_frames(model, helpers.odata_to_block(model, d0), P, H, 2, 2, jacobian=False)
    assert np.abs(r1[..., 18:] - r0[..., 18:]).max() > 1e-3


# ---- the restatement against a finite difference in time -------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("anymal", "links"), ("lumped", "frames"), ("cartpole", "frames"), ("chain9f", "links")])
@pytest.mark.parametrize("I", [0, 1, 2])
@pytest.mark.parametrize("O", [0, 1, 2])
def test_restatement_bias_is_the_time_derivative_of_the_velocity(name, which, I, O):
    model = model_of(name)
    d = with_rep(model, cr.random_data(model, 3, seed=12), I)
    P, H = targets(model, which)
    h = 1e-5
    vp = fr.restate(model, with_rep(model, fr.advance(model, d, I, h), I), P, H, I, O)["v"]
    vm = fr.restate(model, with_rep(model, fr.advance(model, d, I, -h), I), P, H, I, O)["v"]
    a = fr.restate(model, d, P, H, I, O)["a"]
    assert rel((vp - vm) / (2 * h), a) < 1e-6


# ---- host logic -------------------------------------------------------------------------------------------------------
def test_name_and_index_maps():
    model = model_of("lumped")
    nL = model.number_of_links()
    names = model.frame_names()
    assert len(names) > 0
    idx = js.frame.names_to_idxs(model, frame_names=names)
    np.testing.assert_array_equal(idx, np.arange(nL, nL + len(names)))
    assert js.frame.idxs_to_names(model, frame_indices=idx) == tuple(names)
    for f, nm in enumerate(names):
        assert js.frame.idx_of_parent_link(model, frame_index=nL + f) == int(model.kin_dyn_parameters.frame_body[f])
        assert js.frame.idx_to_name(model, frame_index=js.frame.name_to_idx(model, frame_name=nm)) == nm
    lnames = model.link_names()
    np.testing.assert_array_equal(js.link.names_to_idxs(model, link_names=lnames), np.arange(nL))
    assert js.link.idxs_to_names(model, link_indices=np.arange(nL)) == tuple(lnames)
    jnames = model.joint_names()
    np.testing.assert_array_equal(js.joint.names_to_idxs(model, joint_names=jnames), np.arange(len(jnames)))
    assert js.joint.idxs_to_names(model, joint_indices=np.arange(len(jnames))) == tuple(jnames)
    assert js.link.mass(model, link_index=1) == pytest.approx(float(model.kin_dyn_parameters.link_mass[1]))


def test_out_of_range_indices_raise():
    model = model_of("lumped")
    nL, nF = model.number_of_links(), len(model.frame_names())
    for bad in (-1, nL - 1, nL + nF):
        with pytest.raises(ValueError):
            js.frame.idx_of_parent_link(model, frame_index=bad)
        with pytest.raises(ValueError):
            js.frame.idx_to_name(model, frame_index=bad)
    with pytest.raises(ValueError):
        js.frame.name_to_idx(model, frame_name="no such frame")
    with pytest.raises(ValueError):
        js.link.idx_to_name(model, link_index=nL)
    with pytest.raises(ValueError):
        js.link.name_to_idx(model, link_name="no such link")
    with pytest.raises(ValueError):
        js.joint.idx_to_name(model, joint_index=model.number_of_joints())


def test_joint_position_limits():
    model = model_of("anymal")
    kdp = model.kin_dyn_parameters
    lo, hi = js.joint.position_limits(model)
    np.testing.assert_array_equal(lo, kdp.position_limits_min)
    np.testing.assert_array_equal(hi, kdp.position_limits_max)
    names = model.joint_names()[2:5]
    lo3, hi3 = js.joint.position_limits(model, joint_names=names)
    np.testing.assert_array_equal(lo3, kdp.position_limits_min[2:5])
    assert js.joint.position_limit(model, joint_index=3) == (float(kdp.position_limits_min[3]), float(kdp.position_limits_max[3]))
    lo0, hi0 = js.joint.position_limits(model, joint_names=[])
    assert lo0.shape == (0,) and hi0.shape == (0,)
