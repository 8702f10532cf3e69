"""TEST INFRASTRUCTURE for the frame queries (js.link, js.frame, js.model.link_bias_accelerations, js.com.bias_acceleration).

``restate(model, d, parent_links, L_H_F, I, O)`` states the reference's definitions in NumPy float64 for an oracle
data object ``d`` (``oracle.refstep.OracleData``) and a list of targets (parent link, L_H_F):

* the pose ``W_H_F = W_H_L L_H_F`` from the oracle's cached link transforms (``frame.py:148-184``);
* the Jacobian the way ``frame.py:233-315`` composes it: the parent link's Jacobian with Body output
  (``oracle.refrigid.generalized_free_floating_jacobian``), then ``W_X_L``, ``F_X_L`` or ``FW_X_L``;
* the velocity ``O_J I_nu``;
* the bias acceleration: the body-fixed forward recursion of ``link_bias_accelerations`` (``model.py:2179-2395``) over
  the oracle's joint transforms, started from the zero base acceleration of ``I`` converted to inertial-fixed; a frame
  moves with its parent (``F_a = F_X_L L_a``); the output conversion is ``body_to_other_representation`` applied to F.

Representations are the product's integer codes (0 Inertial, 1 Body, 2 Mixed).
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import VelRepr
from oracle import refmath as rm
from oracle import refrigid as rr
from oracle import refstep as rs

REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)  # index = the product's code


def _mv(X, v):
    return np.einsum("...ij,...j->...i", X, v)


def link_bias_body(model, d, I):
    """``(L_a [N, nL, 6], L_v [N, nL, 6])``: body-fixed link bias accelerations and velocities of the reference's
    recursion (model.py:2203-2343) for the generalized velocity in representation ``I``."""
    kdp = model.kin_dyn_parameters
    W_H_B = d.base_transform.astype(np.float64)
    N, nL = W_H_B.shape[0], kdp.number_of_links()
    W_v_WB = np.concatenate([d.base_linear_velocity, d.base_angular_velocity], -1).astype(np.float64)
    rep = REPS[I]
    if rep == VelRepr.Mixed:  # W_vdot_WB = W_X_BW (0 + vx(BW_v_W_BW) BW_v_WB)
        W_H_BW = W_H_B.copy()
        W_H_BW[:, :3, :3] = np.eye(3)
        BW_v_WB = rs.inertial_to_other_representation(W_v_WB, VelRepr.Mixed, W_H_B, is_force=False)
        BW_v_W_BW = np.zeros((N, 6))
        BW_v_W_BW[:, :3] = BW_v_WB[:, :3]
        W_a_B = _mv(rm.adjoint_from_transform(W_H_BW), _mv(rm.vx(BW_v_W_BW), BW_v_WB))
    else:  # (Inertial: W_v_WC = 0; Body: the cross product of B_v_WB with itself)
        W_a_B = np.zeros((N, 6))
    s = d.joint_positions.astype(np.float64)
    sd = d.joint_velocities.astype(np.float64)
    i_X_l = rs.joint_transforms(model, s, W_H_B)
    S = kdp.motion_subspaces.astype(np.float64)
    lam = kdp.parent_array
    v = np.zeros((N, nL, 6))
    a = np.zeros((N, nL, 6))
    v[:, 0] = rs.inertial_to_other_representation(W_v_WB, VelRepr.Body, W_H_B, is_force=False)
    a[:, 0] = _mv(rm.adjoint_from_transform(W_H_B, inverse=True), W_a_B)
    for i in range(1, nL):
        vJ = S[i].reshape(6)[None] * sd[:, i - 1, None]
        v[:, i] = _mv(i_X_l[:, i], v[:, lam[i]]) + vJ
        a[:, i] = _mv(i_X_l[:, i], a[:, lam[i]]) + _mv(rm.vx(v[:, i]), vJ)
    return a, v


def restate(model, d, parent_links, L_H_F, I, O):
    """Every output of the frame kernel for the targets: ``dict(H [N, nt, 4, 4], v [N, nt, 6], J [N, nt, 6, 6+n],
    a [N, nt, 6])`` in float64 (``a`` = ``O_Jdot_WF_I I_nu``)."""
    parent = np.asarray(parent_links, dtype=int).reshape(-1)
    L_H_F = np.asarray(L_H_F, dtype=np.float64).reshape(-1, 4, 4)
    W_H_L = d.link_transforms.astype(np.float64)[:, parent]  # [N, nt, 4, 4]
    W_H_F = W_H_L @ L_H_F[None]
    F_H_L = rm.transform_inverse(W_H_F) @ W_H_L
    L_J = rr.generalized_free_floating_jacobian(model, d, REPS[I], VelRepr.Body).astype(np.float64)[:, parent]
    L_a, L_v = link_bias_body(model, d, I)
    L_a, L_v = L_a[:, parent], L_v[:, parent]
    F_X_L = rm.adjoint_from_transform(F_H_L)
    F_a, F_v = _mv(F_X_L, L_a), _mv(F_X_L, L_v)
    rep = REPS[O]
    if rep == VelRepr.Inertial:
        O_X_F = rm.adjoint_from_transform(W_H_F)
        cross = np.zeros_like(F_v)
    elif rep == VelRepr.Body:
        O_X_F = np.broadcast_to(np.eye(6), F_X_L.shape)
        cross = np.zeros_like(F_v)
    else:
        FW_H_F = W_H_F.copy()
        FW_H_F[..., :3, 3] = 0.0
        O_X_F = rm.adjoint_from_transform(FW_H_F)
        F_v_FW_F = F_v.copy()
        F_v_FW_F[..., :3] = 0.0  # body-fixed velocity of F relative to FW: the angular part
        cross = _mv(rm.vx(F_v_FW_F), F_v)
    O_J = O_X_F @ F_X_L @ L_J
    nu = d.generalized_velocity(REPS[I]).astype(np.float64)
    return dict(H=W_H_F, J=O_J, v=np.einsum("ntij,nj->nti", O_J, nu), a=_mv(O_X_F, F_a + cross))


def link_targets(model):
    nL = model.number_of_links()
    return np.arange(nL), np.broadcast_to(np.eye(4), (nL, 4, 4))


def frame_targets(model):
    kdp = model.kin_dyn_parameters
    return np.asarray(kdp.frame_body), np.asarray(kdp.frame_transform, np.float64)


# ---- a finite difference in time (tests/test_frames_cpu.py, tests/test_frames_gpu.py) ----------------------------------------
def advance(model, d, I, h):
    """The state after time h at constant I_nu (s'' = 0; the base moves with constant velocity in representation I)."""
    W_H_B = d.base_transform.astype(np.float64)
    nu = d.generalized_velocity(REPS[I]).astype(np.float64)
    vB, w = nu[:, :3], nu[:, 3:6]
    R, p = W_H_B[:, :3, :3], W_H_B[:, :3, 3]
    if I == 0:  # constant W_v_WB: a screw motion, H(t) = expm(t [w]^ ; t v) H(0)
        X = np.zeros((d.batch_size, 4, 4))
        X[:, :3, :3] = rm.wedge(w) * h
        X[:, :3, 3] = vB * h
        H = np.stack([_expm(x) for x in X]) @ W_H_B
    elif I == 1:  # constant B_v_WB: H(t) = H(0) expm(t [w]^ ; t v)
        X = np.zeros((d.batch_size, 4, 4))
        X[:, :3, :3] = rm.wedge(w) * h
        X[:, :3, 3] = vB * h
        H = W_H_B @ np.stack([_expm(x) for x in X])
    else:  # constant mixed velocity: p(t) = p + t pdot, R(t) = expm(t [w]^) R
        H = W_H_B.copy()
        H[:, :3, 3] = p + h * vB
        H[:, :3, :3] = np.stack([_expm3(x) for x in rm.wedge(w) * h]) @ R
    q = np.stack([_quat(Rk) for Rk in H[:, :3, :3]])
    s = d.joint_positions.astype(np.float64) + h * d.joint_velocities.astype(np.float64)
    W_v = rs.other_representation_to_inertial(nu[:, :6], REPS[I], H, is_force=False)
    out = dataclasses.replace(d, base_position=H[:, :3, 3].copy(), base_quaternion=q, joint_positions=s,
                              base_linear_velocity=W_v[:, :3].copy(), base_angular_velocity=W_v[:, 3:].copy())  # fmt: skip
    return out.update_caches(model)


def _expm(X):
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ X / k
        out = out + term
    return out


def _expm3(X):
    return _expm(np.pad(X, ((0, 1), (0, 1))))[:3, :3]


def _quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0, R[1, 0] - R[0, 1])
    return np.array([w, x, y, z])
