"""``jaxsim.api.link`` mirror (``src/jaxsim/api/link.py``): names, inertial parameters and the kinematics of the links.

``transform``, ``velocity``, ``jacobian`` and ``bias_acceleration`` come from one launch of the frame kernel over the
table of all links (``api/frame.py``), cached on the data object; ``jacobian_derivative`` is the reference's host
composition over the Jacobian kernel.  Link indices are integers; ``name_to_idx`` translates a name.
"""

from __future__ import annotations

import numpy as np

from ..model import VelRepr
from . import frame as _frame


# ---- names and indices (link.py:19-113) -----------------------------------------------------------------------------
def _check(model, link_index) -> int:
    i = int(link_index)
    if i < 0 or i >= model.number_of_links():
        raise ValueError(f"Invalid link index '{i}'")
    return i


def name_to_idx(model, *, link_name: str) -> int:
    """``name_to_idx`` (link.py:19-42)."""
    names = model.link_names()
    if link_name not in names:
        raise ValueError(f"Link '{link_name}' not found in the model")
    return names.index(link_name)


def idx_to_name(model, *, link_index) -> str:
    """``idx_to_name`` (link.py:45-68)."""
    return model.link_names()[_check(model, link_index)]


def names_to_idxs(model, *, link_names) -> np.ndarray:
    """``names_to_idxs`` (link.py:71-92)."""
    return np.array([name_to_idx(model, link_name=nm) for nm in link_names], dtype=int)


def idxs_to_names(model, *, link_indices) -> tuple[str, ...]:
    """``idxs_to_names`` (link.py:95-113)."""
    return tuple(idx_to_name(model, link_index=i) for i in np.asarray(link_indices).reshape(-1))


# ---- inertial parameters (link.py:116-160) --------------------------------------------------------------------------
def mass(model, *, link_index) -> float:
    """``mass`` (link.py:116-133)."""
    return float(model.kin_dyn_parameters.link_mass[_check(model, link_index)])


def spatial_inertia(model, *, link_index) -> np.ndarray:
    """``spatial_inertia`` (link.py:136-160): the 6x6 inertia in the link frame."""
    from .model import link_spatial_inertia_matrices

    return np.asarray(link_spatial_inertia_matrices(model))[_check(model, link_index)]


# ---- kinematics (link.py:163-460) -----------------------------------------------------------------------------------
def _rep(data, output_vel_repr):
    return data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)


def _inertial_base_offset(model, data):
    """The kernel places an Inertial output at the pose of the cached link kinematics (the reference's frame.py and
    link_bias_accelerations do); the reference's LINK Jacobian places it at the base pose of the dynamics (W_X_B B_J).
    They differ by the base-link offset R_B d of quirk 12: [N, 3], zero for most models."""
    d = np.asarray(model.kin_dyn_parameters.suc_H_i[0][:3, 3], dtype=np.float64)
    if not d.any():
        return None
    return np.einsum("nij,j->ni", data._base_transform_batched()[:, :3, :3], d)


def transform(model, data, *, link_index):
    """``transform`` (link.py:163-187): ``W_H_L``, [4, 4] / [N, 4, 4]."""
    L = _check(model, link_index)
    rec, _ = _frame._record(model, data, _frame._ALL_LINKS, data.velocity_representation)
    return data._out(_frame._pose(rec[:, L]).astype(data.dtype))


def com_position(model, data, *, link_index, in_link_frame: bool = True):
    """``com_position`` (link.py:190-222): the CoM of the link in its own frame, or in the world frame."""
    L = _check(model, link_index)
    c = np.asarray(model.kin_dyn_parameters.link_com[L], dtype=np.float64)
    if in_link_frame:
        return data._out(np.broadcast_to(c, (data.batch_size, 3)).astype(data.dtype))
    H = _frame._pose(_frame._record(model, data, _frame._ALL_LINKS, data.velocity_representation)[0][:, L])
    return data._out((np.einsum("nij,j->ni", H[:, :3, :3], c) + H[:, :3, 3]).astype(data.dtype))


def velocity(model, data, *, link_index, output_vel_repr=None):
    """``velocity`` (link.py:353-393): ``O_v_WL = O_J_WL_I I_nu``, [6] / [N, 6]."""
    L = _check(model, link_index)
    out_rep = _rep(data, output_vel_repr)
    rec, _ = _frame._record(model, data, _frame._ALL_LINKS, out_rep)
    v = rec[:, L, _frame.VEL : _frame.VEL + 6].copy()
    off = _inertial_base_offset(model, data) if out_rep == VelRepr.Inertial else None
    if off is not None:
        v[:, :3] -= np.cross(off, v[:, 3:])
    return data._out(v.astype(data.dtype))


def jacobian(model, data, *, link_index, output_vel_repr=None):
    """``jacobian`` (link.py:225-350): ``O_J_WL_I``, [6, 6+n] / [N, 6, 6+n]."""
    L = _check(model, link_index)
    out_rep = _rep(data, output_vel_repr)
    _, J = _frame._record(model, data, _frame._ALL_LINKS, out_rep, jacobian=True)
    J = J[:, L].copy()
    off = _inertial_base_offset(model, data) if out_rep == VelRepr.Inertial else None
    if off is not None:
        J[:, :3] -= np.cross(off[:, :, None], J[:, 3:], axis=1)
    return data._out(J.astype(data.dtype))


def bias_acceleration(model, data, *, link_index, output_vel_repr=None):
    """``bias_acceleration`` (link.py:463-494): ``O_Jdot_WL_I I_nu``, [6] / [N, 6].  With the output in the data's
    representation this is row ``link_index`` of ``js.model.link_bias_accelerations``."""
    L = _check(model, link_index)
    rec, _ = _frame._record(model, data, _frame._ALL_LINKS, _rep(data, output_vel_repr))
    return data._out(rec[:, L, _frame.BIAS : _frame.BIAS + 6].astype(data.dtype))


def jacobian_derivative(model, data, *, link_index, output_vel_repr=None):
    """``jacobian_derivative`` (link.py:396-460): ``O_Jdot_WL_I``, [6, 6+n] / [N, 6, 6+n] -- row ``link_index`` of
    ``js.model.generalized_free_floating_jacobian_derivative``, a host composition over the Jacobian kernel (independent of
    the frame kernel)."""
    from .model import generalized_free_floating_jacobian_derivative

    L = _check(model, link_index)
    Jd = np.asarray(generalized_free_floating_jacobian_derivative(model, data, output_vel_repr=_rep(data, output_vel_repr)))
    return Jd[..., L, :, :]
