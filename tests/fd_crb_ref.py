"""TEST INFRASTRUCTURE for ``js.model.forward_dynamics_crb`` (MODE_FD_CRB).

``forward_dynamics_crb(model, d, joint_forces=, link_forces=)`` restates the reference's CRB path (``api/model.py:1409-1498``)
in NumPy float64 for an oracle data object ``d`` (``oracle.refstep.OracleData``), in ``d.velocity_representation``:

* ``M`` and ``h`` from ``oracle.refstep`` (``free_floating_mass_matrix``, ``free_floating_bias_forces``);
* ``J^T f`` from the link Jacobians with the data's representation on both sides
  (``oracle.refrigid.generalized_free_floating_jacobian``, as ``tests/frames_ref.py`` uses it): the reference's
  ``generalized_free_floating_jacobian`` -- the wrench of every link acts where the CACHED link transforms place the link;
* ``numpy.linalg.solve`` on the whole matrix (floating base) or on its joint block with a zero base acceleration (fixed
  base), the reference's two branches.

For a model whose base link has a pose offset (``KParams::has_base_off``, DESIGN.md "quirk 12") the reference's ABA and
RNEA move an external wrench with their own, offset-free link frames, while the Jacobians follow the cached transforms;
``link_forces_differ_from_aba(model)`` names those models.  The product's kernel follows the CRB path, like this file.
"""

from __future__ import annotations

import numpy as np

from oracle import refrigid as rr
from oracle import refstep as rs


def generalized_forces(model, d, link_forces):
    """``J^T f`` [N, 6+n]: ``link_forces`` [N, nL, 6] in the data's representation."""
    rep = d.velocity_representation
    J = rr.generalized_free_floating_jacobian(model, d, rep, rep).astype(np.float64)  # [N, nL, 6, 6+n]
    return np.einsum("nlag,nla->ng", J, np.asarray(link_forces, np.float64))


def forward_dynamics_crb(model, d, *, joint_forces=None, link_forces=None):
    """``(base acceleration [N, 6] in d.velocity_representation, joint accelerations [N, n])``."""
    N, n = d.batch_size, model.dofs()
    tau = np.zeros((N, n)) if joint_forces is None else np.asarray(joint_forces, np.float64).reshape(N, n)
    M = rs.free_floating_mass_matrix(model, d).astype(np.float64)
    h = rs.free_floating_bias_forces(model, d).astype(np.float64)
    rhs = np.concatenate([np.zeros((N, 6)), tau], -1) - h
    if link_forces is not None:
        rhs = rhs + generalized_forces(model, d, link_forces)
    if model.floating_base():
        nud = np.linalg.solve(M, rhs[..., None])[..., 0]
        return nud[:, :6], nud[:, 6:]
    sdd = np.linalg.solve(M[:, 6:, 6:], rhs[:, 6:, None])[..., 0] if n else np.zeros((N, 0))
    return np.zeros((N, 6)), sdd


def link_forces_differ_from_aba(model) -> bool:
    """True for a model whose base link carries a pose offset: ``forward_dynamics_crb`` and ``forward_dynamics_aba`` of
    the reference then treat external link wrenches differently (the module docstring)."""
    return bool(np.any(np.abs(np.asarray(model.kin_dyn_parameters.suc_H_i[0][:3, 3], np.float64)) > 0))
