"""TEST INFRASTRUCTURE for the centroidal queries (js.com, js.model momentum / energy functions).

* ``restate(model, d)``: the reference's definitions (``src/jaxsim/api/com.py``; ``src/jaxsim/api/model.py:888-925,
  1988-2175, 2397-2453``) written out the way the reference composes them -- the body-fixed mass matrix of the oracle's
  CRBA (``oracle.refstep.crba``), the cached link transforms of ``OracleData.update_caches`` and the reference's 6x6
  adjoints -- in NumPy float64, for the data's velocity representation.
* ``pin(text, ...)``: an independent statement from the URDF TEXT (``tests/maxcoord.py``'s parser and rotation helpers):
  every massive URDF body placed by its own kinematics, the quantities as plain sums over bodies.
"""

from __future__ import annotations

import numpy as np

import maxcoord
import oracle
from oracle import VelRepr
from oracle import refmath as rm
from oracle import refstep as rs

_REPS = (VelRepr.Inertial, VelRepr.Body, VelRepr.Mixed)


def _blockdiag(X, n):
    T = np.zeros(X.shape[:-2] + (6 + n, 6 + n))
    T[..., :6, :6] = X
    T[..., 6:, 6:] = np.eye(n)
    return T


def _translation(p):
    H = np.broadcast_to(np.eye(4), p.shape[:-1] + (4, 4)).copy()
    H[..., :3, 3] = p
    return H


def com_position(model, d):
    """``com_position`` (com.py:12-51) from the cached link transforms."""
    kdp = model.kin_dyn_parameters
    m = kdp.link_mass.astype(np.float64)
    H = d.link_transforms.astype(np.float64)
    p = np.einsum("nlij,lj->nli", H[..., :3, :3], kdp.link_com.astype(np.float64)) + H[..., :3, 3]
    return np.einsum("l,nli->ni", m, p) / m.sum()


def total_momentum_jacobian(model, d, rep, out_rep):
    """``total_momentum_jacobian`` (model.py:2024-2087) with the data in ``rep``: the general path of the reference
    (Body mass matrix, input and output transforms)."""
    n = model.dofs()
    M_B = rs.crba(model, joint_positions=d.joint_positions.astype(np.float64))
    B_Jh_B = M_B[:, :6]
    W_H_B = d.base_transform.astype(np.float64)
    BW_H_B = W_H_B.copy()
    BW_H_B[:, :3, 3] = 0.0
    if rep == VelRepr.Body:
        B_Jh = B_Jh_B
    elif rep == VelRepr.Inertial:
        B_Jh = B_Jh_B @ _blockdiag(rm.adjoint_from_transform(W_H_B, inverse=True), n)
    else:
        B_Jh = B_Jh_B @ _blockdiag(rm.adjoint_from_transform(BW_H_B, inverse=True), n)
    if out_rep == VelRepr.Body:
        return B_Jh
    if out_rep == VelRepr.Inertial:
        return np.swapaxes(rm.adjoint_from_transform(W_H_B, inverse=True), -1, -2) @ B_Jh
    return np.swapaxes(rm.adjoint_from_transform(BW_H_B, inverse=True), -1, -2) @ B_Jh


def restate(model, d, rep):
    """Every quantity of the feature for the data ``d`` (OracleData) read in representation ``rep``: a dict of float64
    arrays with a leading batch axis; ``*_jacobian_out`` are dicts over the output representation."""
    n = model.dofs()
    W_H_B = d.base_transform.astype(np.float64)
    R = W_H_B[:, :3, :3]
    m = float(model.kin_dyn_parameters.link_mass.sum())
    p_com = com_position(model, d)
    nu = d.generalized_velocity(rep).astype(np.float64)
    M_B = rs.crba(model, joint_positions=d.joint_positions.astype(np.float64))
    out = {"com_position": p_com}
    # com.py:111-158 / 161-195: G = G[W] for Inertial and Mixed, G[B] for Body
    W_H_G = _translation(p_com) if rep != VelRepr.Body else W_H_B.copy()
    W_H_G[:, :3, 3] = p_com
    B_H_G = rm.transform_inverse(W_H_B) @ W_H_G
    G_Xf_B = np.swapaxes(rm.adjoint_from_transform(B_H_G), -1, -2)
    B_Jh = total_momentum_jacobian(model, d, rep, VelRepr.Body)
    G_J = G_Xf_B @ B_Jh
    B_Xv_G = rm.adjoint_from_transform(B_H_G)
    G_Mbb = np.swapaxes(B_Xv_G, -1, -2) @ M_B[:, :6, :6] @ B_Xv_G
    G_avgJ = np.linalg.inv(G_Mbb) @ G_J
    out["centroidal_momentum_jacobian"] = G_J
    out["centroidal_momentum"] = np.einsum("nij,nj->ni", G_J, nu)
    out["locked_centroidal_spatial_inertia"] = G_Mbb
    out["average_centroidal_velocity_jacobian"] = G_avgJ
    out["average_centroidal_velocity"] = np.einsum("nij,nj->ni", G_avgJ, nu)
    out["com_linear_velocity"] = out["average_centroidal_velocity"][:, :3]
    # model.py:1988-2157
    Jh = total_momentum_jacobian(model, d, rep, rep)
    out["total_momentum_jacobian_out"] = {o: total_momentum_jacobian(model, d, rep, o) for o in _REPS}
    out["total_momentum"] = np.einsum("nij,nj->ni", Jh, nu)
    out["locked_spatial_inertia"] = Jh[:, :, :6]
    avg = {}
    for o in _REPS:
        if o == VelRepr.Inertial:
            X = rm.adjoint_from_transform(_translation(p_com))
        elif o == VelRepr.Body:
            X = rm.adjoint_from_transform(_translation(np.einsum("nji,nj->ni", R, p_com - W_H_B[:, :3, 3])))
        else:
            X = rm.adjoint_from_transform(_translation(p_com - W_H_B[:, :3, 3]))
        avg[o] = X @ G_avgJ
    out["average_velocity_jacobian_out"] = avg
    out["average_velocity"] = np.einsum("nij,nj->ni", avg[rep], nu)
    # model.py:2397-2453
    nu_B = d.generalized_velocity(VelRepr.Body).astype(np.float64)
    K = 0.5 * np.einsum("ni,nij,nj->n", nu_B, M_B, nu_B)
    U = m * p_com[:, 2] * model.gravity
    out.update(kinetic_energy=K, potential_energy=U, mechanical_energy=K + U)
    out["link_spatial_inertia_matrices"] = rs._link_spatial_inertia(model, np.float64)
    return out


def pin(text, model, d):
    """From the URDF text: ``dict(m, com [N,3], h [N,6] in G[W], K [N], locked [N,6,6] in G[W])`` -- the base link
    placed at the state's base pose, moving with the stored (mixed) base velocity, fixed bases included."""
    U = maxcoord.Urdf(text)
    jn = model.joint_names()
    N = d.base_position.shape[0]
    bv = d.base_velocity(VelRepr.Mixed).astype(np.float64)
    res = dict(com=np.zeros((N, 3)), h=np.zeros((N, 6)), K=np.zeros(N), locked=np.zeros((N, 6, 6)))
    bodies = [b for b, rec in U.links.items() if rec["mass"] > 0.0]
    res["m"] = sum(U.links[b]["mass"] for b in bodies)
    for e in range(N):
        s = dict(zip(jn, d.joint_positions[e].astype(np.float64)))
        sd = dict(zip(jn, d.joint_velocities[e].astype(np.float64)))
        pose = {U.base: (d.base_position[e].astype(np.float64), maxcoord.quat_matrix(d.base_quaternion[e].astype(np.float64)))}
        vel = {U.base: (bv[e, :3], bv[e, 3:])}
        stack = [U.base]
        while stack:
            par = stack.pop()
            oP, RP = pose[par]
            vP, wP = vel[par]
            for name in U.by_parent.get(par, []):
                j = U.joints[name]
                Rj, oj = RP @ j["R"], oP + RP @ j["xyz"]
                u = Rj @ j["axis"]
                q, qd = (s.get(name, 0.0), sd.get(name, 0.0)) if j["type"] != "fixed" else (0.0, 0.0)
                if j["type"] == "revolute":
                    RC, oC, wC, vC = Rj @ maxcoord.axis_angle_matrix(j["axis"], q), oj, wP + u * qd, vP + np.cross(wP, oj - oP)
                elif j["type"] == "prismatic":
                    RC, oC = Rj, oj + u * q
                    wC, vC = wP, vP + np.cross(wP, oC - oP) + u * qd
                else:
                    RC, oC, wC, vC = Rj, oj, wP, vP + np.cross(wP, oj - oP)
                pose[j["child"]], vel[j["child"]] = (oC, RC), (vC, wC)
                stack.append(j["child"])
        c, v, w, Iw, mm = [], [], [], [], []
        for b in bodies:
            L = U.links[b]
            o, Rb = pose[b]
            ci = o + Rb @ L["com"]
            c.append(ci)
            w.append(vel[b][1])
            v.append(vel[b][0] + np.cross(vel[b][1], ci - o))
            Iw.append(Rb @ L["Rin"] @ L["I"] @ L["Rin"].T @ Rb.T)
            mm.append(L["mass"])
        pG = sum(mi * ci for mi, ci in zip(mm, c)) / res["m"]
        h = np.zeros(6)
        locked = np.zeros((6, 6))
        locked[:3, :3] = res["m"] * np.eye(3)
        K = 0.0
        for mi, ci, vi, wi, Ii in zip(mm, c, v, w, Iw):
            h[:3] += mi * vi
            h[3:] += Ii @ wi + np.cross(ci - pG, mi * vi)
            K += 0.5 * mi * vi @ vi + 0.5 * wi @ Ii @ wi
            S = maxcoord.skew(ci - pG)
            locked[3:, 3:] += Ii + mi * S @ S.T
        res["com"][e], res["h"][e], res["K"][e], res["locked"][e] = pG, h, K, locked
    return res


def random_data(model, N, seed, dtype=np.float64, rep=VelRepr.Mixed, base_velocity=True, far=False):
    """Random states; a fixed-base model keeps a NON-ZERO stored base velocity (the reference's nu includes it) unless
    ``base_velocity=False``; ``far``: the base 1 km from the origin."""
    kw = dict(base_pos_bounds=((999.0, -1001.0, 999.5), (1001.0, -999.0, 1000.5))) if far else {}
    d = oracle.random_model_data(model, batch_size=N, seed=seed, dtype=dtype, velocity_representation=rep, **kw)
    rng = np.random.default_rng(seed + 7)
    if base_velocity:
        d.base_linear_velocity[:] = rng.uniform(-1, 1, d.base_linear_velocity.shape).astype(dtype)
        d.base_angular_velocity[:] = rng.uniform(-1, 1, d.base_angular_velocity.shape).astype(dtype)
    else:
        d.base_linear_velocity[:] = 0
        d.base_angular_velocity[:] = 0
    return d.update_caches(model)
