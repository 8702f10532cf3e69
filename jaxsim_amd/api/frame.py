"""``jaxsim.api.frame`` mirror (``src/jaxsim/api/frame.py``): poses, velocities, Jacobians and bias accelerations of the
model frames, from ONE launch of the frame kernel (``jxs_frame_kinematics``, ``MODE_FRAMES``).

A target of the kernel is a (parent link, ``L_H_F``) pair; a link is the target (link, identity).  Per target and
environment the kernel writes a record of ``JXS_FRAME_ROWS`` rows -- ``W_H_F`` as [R|p], ``O_v_WF`` and
``O_Jdot_WF_I I_nu`` -- and on request the Jacobian ``O_J_WF_I`` [6, 6+n]; ``I`` is the data's velocity representation,
``O`` the output representation.  Two target tables live on every device model: all links, and all model frames.  The
host copy of a record is cached on the data object per (table, I, O, Jacobian), so ``transform`` followed by
``velocity`` on the same state is one launch.  Frame indices start at the number of links, as in the reference.
``jacobian_derivative`` is a host composition over the Jacobian kernel (``MODE_JAC``), like the reference's.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, runtime
from ..model import VelRepr
from ..runtime import DeviceArray

# include/jaxsim_amd.h JXS_FRAME_*: rows of the record of one target
ROWS = 24
POSE, VEL, BIAS = 0, 12, 18
MAX_TARGETS = 4096

_ALL_LINKS, _ALL_FRAMES = "links", "frames"


class Targets:
    """An immutable target table on the device (``jxs_frames``), freed with this object."""

    def __init__(self, dm, parent_links, L_H_F):
        parent = np.ascontiguousarray(parent_links, dtype=np.int32).reshape(-1)
        H = np.ascontiguousarray(L_H_F, dtype=np.float64).reshape(-1, 4, 4)
        if H.shape[0] != parent.shape[0]:
            raise ValueError((H.shape, parent.shape))
        h = C.c_void_p()
        _lib.check(
            _lib.load().jxs_frames_create(dm.handle, int(parent.shape[0]), parent.ctypes.data_as(C.POINTER(C.c_int32)),
                                          H.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)),  # fmt: skip
            "jxs_frames_create",
        )
        self.handle, self.n, self._dm = h, int(parent.shape[0]), dm  # (keeps the model alive as long as the table)

    def __del__(self):
        try:
            _lib.load().jxs_frames_destroy(self.handle)
        except Exception:
            pass


def _targets_of(model, dm, which):
    """The table of all links / all model frames of a device model, created on first use and freed with it."""
    tables = dm.__dict__.setdefault("_frame_targets", {})
    if which not in tables:
        kdp = model.kin_dyn_parameters
        if which == _ALL_LINKS:
            nL = model.number_of_links()
            tables[which] = Targets(dm, np.arange(nL), np.broadcast_to(np.eye(4), (nL, 4, 4)))
        else:
            if len(kdp.frame_names) == 0:
                raise ValueError("the model has no frames")
            tables[which] = Targets(dm, kdp.frame_body, kdp.frame_transform)
    return tables[which]


def _launch(model, data, targets: Targets, out_rep, jacobian, out=None, out_jacobian=None):
    from .. import specialize

    dm = targets._dm
    specialize.ensure_mode(dm, model, specialize.MODE_FRAMES)  # (first call: cached object, or built when hipcc is there)
    N, n, nt = data.batch_size, model.dofs(), targets.n
    tile = data._state.tile
    rows = nt * ROWS
    out = out if out is not None else DeviceArray(rows, N, data.dtype, tile=tile)
    if (out.rows, out.cols, out.dtype, out.tile) != (rows, N, np.dtype(data.dtype), tile):
        raise ValueError(((out.rows, out.cols, out.dtype), (rows, N, np.dtype(data.dtype))))
    if jacobian:
        jrows = nt * 6 * (6 + n)
        out_jacobian = out_jacobian if out_jacobian is not None else DeviceArray(jrows, N, data.dtype, tile=tile)
        if (out_jacobian.rows, out_jacobian.cols, out_jacobian.dtype, out_jacobian.tile) != (jrows, N, np.dtype(data.dtype), tile):
            raise ValueError(((out_jacobian.rows, out_jacobian.cols, out_jacobian.dtype), (jrows, N, np.dtype(data.dtype))))
    _lib.check(
        _lib.load().jxs_frame_kinematics(dm.handle, targets.handle, C.c_void_p(data._state.ptr), int(data.velocity_representation),
                                         int(out_rep), C.c_void_p(out.ptr), C.c_void_p(out_jacobian.ptr) if jacobian else None,
                                         N, runtime._sp()),  # fmt: skip
        "jxs_frame_kinematics",
    )
    return (out, out_jacobian) if jacobian else out


def kinematics(model, data, frame_names=None, link_names=None, *, output_vel_repr=None, jacobian: bool = False,
               out: DeviceArray | None = None, out_jacobian: DeviceArray | None = None):  # fmt: skip
    """Extension for device-resident loops (like ``js.com.centroidal_quantities``): the record
    ``[n_targets * JXS_FRAME_ROWS][N]`` of ``include/jaxsim_amd.h`` as a ``DeviceArray`` -- and with ``jacobian=True`` the
    pair ``(record, J)``, ``J`` = ``[n_targets * 6 * (6+n)][N]``.  The targets are the given links followed by the given
    frames; with neither given, every link.  One launch, no host round trip; ``out`` / ``out_jacobian`` are reused when
    given.  (A table for a custom selection is created per call: keep the default sets on a hot path.)"""
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    dm = runtime.device_model(model, data.dtype)
    if frame_names is None and link_names is None:
        targets = _targets_of(model, dm, _ALL_LINKS)
    else:
        from . import link as _link

        kdp = model.kin_dyn_parameters
        L = [_link.name_to_idx(model, link_name=nm) for nm in (link_names or ())]
        F = [name_to_idx(model, frame_name=nm) - model.number_of_links() for nm in (frame_names or ())]
        parent = np.array(L + [int(kdp.frame_body[f]) for f in F], dtype=np.int32)
        H = np.concatenate([np.broadcast_to(np.eye(4), (len(L), 4, 4)), np.asarray(kdp.frame_transform, np.float64)[F].reshape(-1, 4, 4)])
        targets = Targets(dm, parent, H)
    return _launch(model, data, targets, out_rep, jacobian, out, out_jacobian)


def _record(model, data, which, out_rep, jacobian=False):
    """``(record [N, n_targets, ROWS], J [N, n_targets, 6, 6+n] or None)`` as float64 host arrays, cached on ``data`` per
    (table, input representation, output representation); the launch with the Jacobian also serves the record."""
    key = (which, int(data.velocity_representation), int(out_rep))
    cache = data._frames
    if cache is None:
        cache = data._frames = {}
    hit = cache.get(key)
    if hit is None or (jacobian and hit[1] is None):
        dm = runtime.device_model(model, data.dtype)
        targets = _targets_of(model, dm, which)
        N, n, nt = data.batch_size, model.dofs(), targets.n
        res = _launch(model, data, targets, out_rep, jacobian)
        rec, J = res if jacobian else (res, None)
        rec_h = rec.to_host().T.astype(np.float64).reshape(N, nt, ROWS)
        J_h = None if J is None else J.to_host().T.astype(np.float64).reshape(N, nt, 6, 6 + n)
        hit = cache[key] = (rec_h, J_h)
    return hit


def _pose(rec):
    H = np.zeros(rec.shape[:-1] + (4, 4))
    H[..., :3, :] = rec[..., POSE : POSE + 12].reshape(rec.shape[:-1] + (3, 4))
    H[..., 3, 3] = 1.0
    return H


# ---- names and indices (frame.py:19-145) ----------------------------------------------------------------------------
def _check_frame_index(model, frame_index) -> int:
    nL, nF = model.number_of_links(), len(model.frame_names())
    i = int(frame_index)
    if i < nL or i >= nL + nF:
        raise ValueError(f"Invalid frame index '{i}'")
    return i


def idx_of_parent_link(model, *, frame_index) -> int:
    """``idx_of_parent_link`` (frame.py:19-45): the link a frame is attached to."""
    i = _check_frame_index(model, frame_index)
    return int(model.kin_dyn_parameters.frame_body[i - model.number_of_links()])


def name_to_idx(model, *, frame_name: str) -> int:
    """``name_to_idx`` (frame.py:48-74): frame indices start at the number of links."""
    names = model.frame_names()
    if frame_name not in names:
        raise ValueError(f"Frame '{frame_name}' not found in the model")
    return model.number_of_links() + names.index(frame_name)


def idx_to_name(model, *, frame_index) -> str:
    """``idx_to_name`` (frame.py:77-103)."""
    return model.frame_names()[_check_frame_index(model, frame_index) - model.number_of_links()]


def names_to_idxs(model, *, frame_names) -> np.ndarray:
    """``names_to_idxs`` (frame.py:106-124)."""
    return np.array([name_to_idx(model, frame_name=nm) for nm in frame_names], dtype=int)


def idxs_to_names(model, *, frame_indices) -> tuple[str, ...]:
    """``idxs_to_names`` (frame.py:127-145)."""
    return tuple(idx_to_name(model, frame_index=i) for i in np.asarray(frame_indices).reshape(-1))


# ---- kinematics (frame.py:148-420) ----------------------------------------------------------------------------------
def transform(model, data, *, frame_index):
    """``transform`` (frame.py:148-184): ``W_H_F = W_H_L L_H_F``, [4, 4] / [N, 4, 4]."""
    f = _check_frame_index(model, frame_index) - model.number_of_links()
    rec, _ = _record(model, data, _ALL_FRAMES, data.velocity_representation)
    return data._out(_pose(rec[:, f]).astype(data.dtype))


def velocity(model, data, *, frame_index, output_vel_repr=None):
    """``velocity`` (frame.py:187-230): ``O_v_WF = O_J_WF_I I_nu``, [6] / [N, 6]."""
    f = _check_frame_index(model, frame_index) - model.number_of_links()
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    rec, _ = _record(model, data, _ALL_FRAMES, out_rep)
    return data._out(rec[:, f, VEL : VEL + 6].astype(data.dtype))


def jacobian(model, data, *, frame_index, output_vel_repr=None):
    """``jacobian`` (frame.py:233-315): ``O_J_WF_I``, [6, 6+n] / [N, 6, 6+n]."""
    f = _check_frame_index(model, frame_index) - model.number_of_links()
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    _, J = _record(model, data, _ALL_FRAMES, out_rep, jacobian=True)
    return data._out(J[:, f].astype(data.dtype))


def bias_acceleration(model, data, *, frame_index, output_vel_repr=None):
    """``O_Jdot_WF_I I_nu`` of a frame, [6] / [N, 6] (the frame counterpart of ``js.link.bias_acceleration``)."""
    f = _check_frame_index(model, frame_index) - model.number_of_links()
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    rec, _ = _record(model, data, _ALL_FRAMES, out_rep)
    return data._out(rec[:, f, BIAS : BIAS + 6].astype(data.dtype))


def _jdot_of_target(model, data, L, W_H_F, out_rep):
    """``O_Jdot_WF_I`` [N, 6, 6+n] of a frame rigidly attached to link ``L`` with pose ``W_H_F`` [N, 4, 4] (frame.py:318-420):
    the Inertial-input, Inertial-output Jacobian of the link and its derivative from the Jacobian kernel, the input
    transform T(I) and its derivative, and the output transform O_X_W and its derivative."""
    from .model import (_adjoint, _block_T, _vx_matrix, generalized_free_floating_jacobian,
                        generalized_free_floating_jacobian_derivative)  # fmt: skip

    N, n = data.batch_size, model.dofs()
    with data.switch_velocity_representation(VelRepr.Inertial):
        W_J = np.asarray(generalized_free_floating_jacobian(model, data, output_vel_repr=VelRepr.Inertial), np.float64)
        W_Jd = np.asarray(generalized_free_floating_jacobian_derivative(model, data, output_vel_repr=VelRepr.Inertial), np.float64)
        W_nu = np.asarray(data.generalized_velocity, np.float64).reshape(N, 6 + n)
    W_J = W_J.reshape(N, -1, 6, 6 + n)[:, L]
    W_Jd = W_Jd.reshape(N, -1, 6, 6 + n)[:, L]
    rep = data.velocity_representation
    W_H_B = data._base_transform_batched()
    if rep == VelRepr.Inertial:
        X, Xd = np.broadcast_to(np.eye(6), (N, 6, 6)), np.zeros((N, 6, 6))
    elif rep == VelRepr.Body:
        W_X_B = _adjoint(W_H_B)
        X, Xd = W_X_B, W_X_B @ _vx_matrix(data._base_velocity_batched(VelRepr.Body))
    else:
        W_H_BW = W_H_B.copy()
        W_H_BW[:, :3, :3] = np.eye(3)
        W_X_BW = _adjoint(W_H_BW)
        BW_v = data._base_velocity_batched(VelRepr.Mixed).copy()
        BW_v[:, 3:] = 0.0
        X, Xd = W_X_BW, W_X_BW @ _vx_matrix(BW_v)
    T, Td = _block_T(X, n), _block_T(Xd, n, identity=False)
    W_v_WF = np.einsum("nij,nj->ni", W_J, W_nu)
    if out_rep == VelRepr.Inertial:
        O_X_W, O_Xd_W = np.broadcast_to(np.eye(6), (N, 6, 6)), np.zeros((N, 6, 6))
    elif out_rep == VelRepr.Body:
        O_X_W = _adjoint(W_H_F, inverse=True)
        O_Xd_W = -O_X_W @ _vx_matrix(W_v_WF)
    else:
        W_H_FW = W_H_F.copy()
        W_H_FW[:, :3, :3] = np.eye(3)
        O_X_W = _adjoint(W_H_FW, inverse=True)
        W_v_W_FW = np.zeros((N, 6))
        W_v_W_FW[:, :3] = W_v_WF[:, :3] + np.cross(W_v_WF[:, 3:], W_H_F[:, :3, 3])  # pdot_F
        O_Xd_W = -O_X_W @ _vx_matrix(W_v_W_FW)
    return O_Xd_W @ W_J @ T + O_X_W @ W_Jd @ T + O_X_W @ W_J @ Td


def jacobian_derivative(model, data, *, frame_index, output_vel_repr=None):
    """``jacobian_derivative`` (frame.py:318-420): ``O_Jdot_WF_I``, [6, 6+n] / [N, 6, 6+n], a host composition over the
    Jacobian kernel (independent of the frame kernel)."""
    f = _check_frame_index(model, frame_index) - model.number_of_links()
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    kdp = model.kin_dyn_parameters
    L = int(kdp.frame_body[f])
    W_H_F = np.asarray(data._kinematics()[0][:, L], np.float64) @ np.asarray(kdp.frame_transform[f], np.float64)
    return data._out(_jdot_of_target(model, data, L, W_H_F, out_rep).astype(data.dtype))
