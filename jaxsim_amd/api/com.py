"""``jaxsim.api.com`` mirror (``src/jaxsim/api/com.py``): centre of mass, centroidal momentum and the locked
centroidal inertia, from ONE launch of the centroidal kernel (``jxs_centroidal``, ``MODE_CENTROIDAL``).

The kernel writes a small record per environment in G[W] = (W_p_CoM, world axes) -- CoM, centroidal momentum,
rotational inertia about the CoM, average centroidal velocity, kinetic and potential energy, mass -- and, on request,
the centroidal momentum matrix ``A_G`` in G[W] for a Mixed generalized velocity.  The reference's frame conventions
are applied on the host, on [N, 6] / [N, 6, 6+n] arrays: G[W] for Inertial and Mixed data, G[B] = (W_p_CoM, base axes)
for Body data.  The host copy of the record is cached on the data object (like its link kinematics): ``com_position``
followed by ``centroidal_momentum`` on the same state is one launch.  ``bias_acceleration`` is composed from the
all-links record of the frame kernel (``api/frame.py``) in Body representation and the link inertias.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, runtime
from ..model import VelRepr
from ..runtime import DeviceArray

# include/jaxsim_amd.h JXS_CENTROIDAL_*: rows of the record
ROWS = 24
COM, MOMENTUM, INERTIA, AVG_VEL, KINETIC, POTENTIAL, MASS = 0, 3, 9, 15, 21, 22, 23


def centroidal_quantities(model, data, *, jacobian: bool = False, out: DeviceArray | None = None,
                          out_jacobian: DeviceArray | None = None):  # fmt: skip
    """Extension for device-resident loops (like ``js.model.gravity_compensation_torques``): the record
    ``[JXS_CENTROIDAL_ROWS][N]`` of ``include/jaxsim_amd.h`` as a ``DeviceArray`` -- and with ``jacobian=True`` the pair
    ``(record, A_G)``, ``A_G`` = ``[6 * (6+n)][N]`` in G[W] for a Mixed generalized velocity.  One launch, no host
    round trip; ``out`` / ``out_jacobian`` are reused when given."""
    from .. import specialize

    dm = runtime.device_model(model, data.dtype)
    specialize.ensure_mode(dm, model, specialize.MODE_CENTROIDAL)  # (first call: cached object, or built when hipcc is there)
    N, n = data.batch_size, model.dofs()
    tile = data._state.tile
    out = out if out is not None else DeviceArray(ROWS, N, data.dtype, tile=tile)
    if (out.rows, out.cols, out.dtype, out.tile) != (ROWS, N, np.dtype(data.dtype), tile):
        raise ValueError(((out.rows, out.cols, out.dtype), (ROWS, N, np.dtype(data.dtype))))
    if jacobian:
        rows = 6 * (6 + n)
        out_jacobian = out_jacobian if out_jacobian is not None else DeviceArray(rows, N, data.dtype, tile=tile)
        if (out_jacobian.rows, out_jacobian.cols, out_jacobian.dtype, out_jacobian.tile) != (rows, N, np.dtype(data.dtype), tile):
            raise ValueError(((out_jacobian.rows, out_jacobian.cols, out_jacobian.dtype), (rows, N, np.dtype(data.dtype))))
    cmm = C.c_void_p(out_jacobian.ptr) if jacobian else None
    _lib.check(
        _lib.load().jxs_centroidal(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), cmm, N, runtime._sp()),
        "jxs_centroidal",
    )
    return (out, out_jacobian) if jacobian else out


def _centroidal(model, data, jacobian: bool = False):
    """``(record [N, ROWS], A_G [N, 6, 6+n] or None)`` as float64 host arrays, cached on ``data`` (the launch with the
    Jacobian also serves the record)."""
    cached = data._cent
    if cached is None or (jacobian and cached[1] is None):
        N, n = data.batch_size, model.dofs()
        res = centroidal_quantities(model, data, jacobian=jacobian)
        rec, J = res if jacobian else (res, None)
        rec_h = rec.to_host().T.astype(np.float64)
        J_h = None if J is None else J.to_host().T.astype(np.float64).reshape(N, 6, 6 + n)
        cached = data._cent = (rec_h, J_h)
    return cached


def _skew(a: np.ndarray) -> np.ndarray:
    S = np.zeros(a.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -a[..., 2], a[..., 1]
    S[..., 1, 0], S[..., 1, 2] = a[..., 2], -a[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -a[..., 1], a[..., 0]
    return S


def _rot6(R: np.ndarray) -> np.ndarray:
    X = np.zeros(R.shape[:-2] + (6, 6))
    X[..., :3, :3] = R
    X[..., 3:, 3:] = R
    return X


def _to_G_frame(data, x: np.ndarray) -> np.ndarray:
    """A G[W] quantity (6-vectors [N, 6] or columns [N, 6, k]) in the data's G frame: G[B] rotates it into base axes."""
    if data.velocity_representation != VelRepr.Body:
        return x
    Rt6 = _rot6(np.swapaxes(data._base_transform_batched()[:, :3, :3], -1, -2))
    return np.einsum("nij,nj->ni", Rt6, x) if x.ndim == 2 else Rt6 @ x


def _base_offset(model, data) -> np.ndarray:
    """R_B d: where the cached kinematics place the base link relative to the base pose of the dynamics (quirk 12 of
    the reference: a translated pose suc_H_i[0] = (1, d) of the base link), [N, 3]."""
    d = np.asarray(model.kin_dyn_parameters.suc_H_i[0][:3, 3], dtype=np.float64)
    return np.einsum("nij,j->ni", data._base_transform_batched()[:, :3, :3], d)


def _locked_G_world(model, data) -> np.ndarray:
    """Locked centroidal inertia in G[W], [N, 6, 6]: diag(m 1, I_G), with the coupling of a base-link offset."""
    rec, _ = _centroidal(model, data)
    N = rec.shape[0]
    m = rec[:, MASS]
    I = rec[:, INERTIA : INERTIA + 6]
    IG = np.stack([I[:, [0, 1, 2]], I[:, [1, 3, 4]], I[:, [2, 4, 5]]], axis=1)
    Se = _skew(-_base_offset(model, data))
    M = np.zeros((N, 6, 6))
    M[:, :3, :3] = m[:, None, None] * np.eye(3)
    M[:, :3, 3:] = m[:, None, None] * np.swapaxes(Se, -1, -2)
    M[:, 3:, :3] = m[:, None, None] * Se
    M[:, 3:, 3:] = IG + m[:, None, None] * (Se @ np.swapaxes(Se, -1, -2))
    return M


def _cmm_mixed_input(model, data) -> np.ndarray:
    """A_G in G[W] for the generalized velocity in the data's representation: A_G^mixed diag(X, 1), v_mixed = X v."""
    from .model import _mixed_to_repr_block

    _, J = _centroidal(model, data, jacobian=True)
    if data.velocity_representation == VelRepr.Mixed:
        return J
    J = J.copy()
    J[:, :, :6] = J[:, :, :6] @ _mixed_to_repr_block(data)
    return J


def com_position(model, data):
    """``com_position`` (``src/jaxsim/api/com.py:12-51``): W_p_CoM, [3] / [N, 3]."""
    rec, _ = _centroidal(model, data)
    return data._out(rec[:, COM : COM + 3].astype(data.dtype))


def centroidal_momentum(model, data):
    """``centroidal_momentum`` (``src/jaxsim/api/com.py:84-108``): in G[W] (Inertial / Mixed data) or G[B] (Body)."""
    rec, _ = _centroidal(model, data)
    return data._out(_to_G_frame(data, rec[:, MOMENTUM : MOMENTUM + 6]).astype(data.dtype))


def centroidal_momentum_jacobian(model, data):
    """``centroidal_momentum_jacobian`` (``src/jaxsim/api/com.py:111-158``), the centroidal momentum matrix:
    [6, 6+n] / [N, 6, 6+n], output in G[W] (Inertial / Mixed data) or G[B] (Body), input in the data's representation."""
    return data._out(_to_G_frame(data, _cmm_mixed_input(model, data)).astype(data.dtype))


def locked_centroidal_spatial_inertia(model, data):
    """``locked_centroidal_spatial_inertia`` (``src/jaxsim/api/com.py:161-195``): [6, 6] / [N, 6, 6] in G[W] or G[B]."""
    M = _locked_G_world(model, data)
    if data.velocity_representation == VelRepr.Body:
        R6 = _rot6(data._base_transform_batched()[:, :3, :3])
        M = np.swapaxes(R6, -1, -2) @ M @ R6
    return data._out(M.astype(data.dtype))


def average_centroidal_velocity(model, data):
    """``average_centroidal_velocity`` (``src/jaxsim/api/com.py:198-221``): M_G^-1 h_G in G[W] or G[B]."""
    rec, _ = _centroidal(model, data)
    return data._out(_to_G_frame(data, rec[:, AVG_VEL : AVG_VEL + 6]).astype(data.dtype))


def average_centroidal_velocity_jacobian(model, data):
    """``average_centroidal_velocity_jacobian`` (``src/jaxsim/api/com.py:224-247``): M_G^-1 A_G, [6, 6+n] / [N, 6, 6+n]."""
    J = np.linalg.solve(_locked_G_world(model, data), _cmm_mixed_input(model, data))
    return data._out(_to_G_frame(data, J).astype(data.dtype))


def com_linear_velocity(model, data):
    """``com_linear_velocity`` (``src/jaxsim/api/com.py:54-81``): the linear part of the average centroidal velocity."""
    rec, _ = _centroidal(model, data)
    return data._out(_to_G_frame(data, rec[:, AVG_VEL : AVG_VEL + 6])[:, :3].astype(data.dtype))


def bias_acceleration(model, data):
    """``bias_acceleration`` (``src/jaxsim/api/com.py:251-421``): the bias linear acceleration of the CoM, [3] / [N, 3], in
    G[W] (Inertial / Mixed data) or G[B] (Body).  The body-fixed link bias accelerations and velocities of the all-links
    record of the frame kernel (input in the data's representation, output Body) give the bias momentum rate
    sum_L W_Xf_L (M_L a_L + v_L x* M_L v_L), whose linear part divided by the mass is the result."""
    from . import frame as _frame
    from .model import link_spatial_inertia_matrices

    rec, _ = _frame._record(model, data, _frame._ALL_LINKS, VelRepr.Body)
    M = np.asarray(link_spatial_inertia_matrices(model), dtype=np.float64)  # [nL, 6, 6]
    a = rec[:, :, _frame.BIAS : _frame.BIAS + 6]
    v = rec[:, :, _frame.VEL : _frame.VEL + 6]
    R = rec[:, :, _frame.POSE : _frame.POSE + 12].reshape(rec.shape[:2] + (3, 4))[..., :3]
    Ma, Mv = np.einsum("lij,nlj->nli", M, a), np.einsum("lij,nlj->nli", M, v)
    f_lin = Ma[..., :3] + np.cross(v[..., 3:], Mv[..., :3])  # linear part of M a + v x* M v
    h_lin = np.einsum("nlij,nlj->ni", R, f_lin)
    acc = h_lin / float(np.sum(model.kin_dyn_parameters.link_mass))
    if data.velocity_representation == VelRepr.Body:
        acc = np.einsum("nji,nj->ni", data._base_transform_batched()[:, :3, :3], acc)
    return data._out(acc.astype(data.dtype))
