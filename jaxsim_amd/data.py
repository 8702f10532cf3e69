"""Batched ``JaxSimModelData`` mirror whose state lives in HBM as one ``[rows][N]`` block.

Mirrors the reference container (``src/jaxsim/api/data.py:46-549``): same field and property
names, base velocity stored inertial-fixed regardless of ``velocity_representation``
(default Mixed, ``:75,151-156,187-188``), normalised ``base_orientation``, cached link
kinematics computed on demand (``_link_transforms`` / ``_link_velocities``, refreshed by a
kernel instead of at every ``replace``).  The object is immutable by convention: ``step``
returns a new one.  Batched inputs have a leading ``N`` axis like the output of
``jax.vmap``; unbatched inputs are treated as ``N = 1`` and squeezed on the way out.
"""

from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _hostmath as hm
from . import _lib, runtime
from .env_specs import CONTACT_FIELDS, CONTACT_ROWS, CONTACT_TIMER_ROWS, DONE_TERMINATED, DONE_TRUNCATED, EVAL_INNERS, EVAL_KINDS, EVAL_OUTERS  # noqa: F401
from .env_specs import ActionSpec, ContactSensorSpec, ObservationSpec, RewardSpec  # (re-exported: jaxsim_amd.data.<Name> are these objects)
from .model import VelRepr
from .state import StateLayout, pack_state, unpack_state


def _inertial_to_other(W_array, rep, W_H_O, is_force):
    """``inertial_to_other_representation`` (``src/jaxsim/api/common.py:100-158``), batched."""
    if rep == VelRepr.Inertial:
        return W_array
    R, p = W_H_O[..., :3, :3], W_H_O[..., :3, 3]
    if rep == VelRepr.Mixed:
        R = np.broadcast_to(np.eye(3), R.shape)
    lin, ang = W_array[..., :3], W_array[..., 3:]
    Rt = np.swapaxes(R, -1, -2)
    if not is_force:  # O_X_W v = [R^T (v - p x w); R^T w]
        return np.concatenate(
            [np.einsum("...ij,...j->...i", Rt, lin - np.cross(p, ang)), np.einsum("...ij,...j->...i", Rt, ang)], -1
        )
    # W_X_O^T f = [R^T f; R^T (mu - p x f)]
    return np.concatenate(
        [np.einsum("...ij,...j->...i", Rt, lin), np.einsum("...ij,...j->...i", Rt, ang - np.cross(p, lin))], -1
    )


def _other_to_inertial(O_array, rep, W_H_O, is_force):
    """``other_representation_to_inertial`` (``src/jaxsim/api/common.py:160-222``), batched."""
    if rep == VelRepr.Inertial:
        return O_array
    R, p = W_H_O[..., :3, :3], W_H_O[..., :3, 3]
    if rep == VelRepr.Mixed:
        R = np.broadcast_to(np.eye(3), R.shape)
    lin = np.einsum("...ij,...j->...i", R, O_array[..., :3])
    ang = np.einsum("...ij,...j->...i", R, O_array[..., 3:])
    if not is_force:  # W_X_O v = [R v + p x R w; R w]
        return np.concatenate([lin + np.cross(p, ang), ang], -1)
    # O_X_W^T f = [R f; R mu + p x R f]
    return np.concatenate([lin, ang + np.cross(p, lin)], -1)


class JaxSimModelData:
    """State of N independent instances of one model, resident on the GPU."""

    def __init__(self, model, state: runtime.DeviceArray, velocity_representation: VelRepr, batched: bool):
        self._model_ref = model
        self._state = state
        self.velocity_representation = velocity_representation if type(velocity_representation) is VelRepr else VelRepr(velocity_representation)
        self._batched = bool(batched)
        self._host = None  # lazily downloaded dict of [N,...] arrays
        self._kin = None  # lazily computed (link_transforms, link_velocities)
        self._cent = None  # lazily computed centroidal record and momentum matrix (api/com.py)
        self._frames = None  # lazily computed frame records per (targets, representations) (api/frame.py)

    # -- construction -----------------------------------------------------------------------
    @staticmethod
    def build(
        model,
        base_position=None,
        base_quaternion=None,
        joint_positions=None,
        base_linear_velocity=None,
        base_angular_velocity=None,
        joint_velocities=None,
        contact_state: dict | None = None,
        velocity_representation: VelRepr = VelRepr.Mixed,
        *,
        batch_size: int | None = None,
        dtype=np.float64,
    ) -> "JaxSimModelData":
        """``JaxSimModelData.build`` (``src/jaxsim/api/data.py:65-202``).

        The base velocity arguments are expressed in ``velocity_representation`` and stored
        inertial-fixed.  ``dtype`` defaults to float64 like the reference (x64 enabled,
        ``src/jaxsim/__init__.py:17-35``); the benchmark configurations use float32.
        """
        lay = StateLayout.of(model)
        n, n_cp = lay.n_joints, lay.n_points
        given = dict(
            base_position=(base_position, 3),
            base_quaternion=(base_quaternion, 4),
            joint_positions=(joint_positions, n),
            base_linear_velocity=(base_linear_velocity, 3),
            base_angular_velocity=(base_angular_velocity, 3),
            joint_velocities=(joint_velocities, n),
        )
        N, batched = (batch_size, True) if batch_size is not None else (1, False)
        for name, (val, width) in given.items():
            if val is None:
                continue
            arr = np.asarray(val, dtype=np.float64)
            if arr.ndim == 2:
                N, batched = arr.shape[0], True
        td = (contact_state or {}).get("tangential_deformation")
        if td is not None and np.ndim(td) == 3:
            N, batched = np.shape(td)[0], True

        def prep(val, width, default=None):
            if val is None:
                out = np.zeros((N, width))
                if default is not None:
                    out[:] = default
                return out
            arr = np.asarray(val, dtype=np.float64)
            arr = np.atleast_1d(arr.squeeze()) if arr.ndim != 2 else arr
            if arr.ndim == 1:
                if arr.shape != (width,):
                    raise ValueError((arr.shape, (width,)))  # like rbda/utils.py:102-133
                arr = np.broadcast_to(arr, (N, width))
            elif arr.shape != (N, width):
                raise ValueError((arr.shape, (N, width)))
            return np.array(arr, dtype=np.float64)

        p = prep(base_position, 3)
        q = prep(base_quaternion, 4, default=[1.0, 0, 0, 0])
        s = prep(joint_positions, n)
        sd = prep(joint_velocities, n)
        vl = prep(base_linear_velocity, 3)
        va = prep(base_angular_velocity, 3)
        W_H_B = np.zeros((N, 4, 4))
        qn = q / np.linalg.norm(q, axis=-1, keepdims=True)
        W_H_B[:, :3, :3] = hm.quaternion_to_rotation(qn)
        W_H_B[:, :3, 3] = p
        W_H_B[:, 3, 3] = 1
        W_v = _other_to_inertial(np.concatenate([vl, va], -1), VelRepr(velocity_representation), W_H_B, False)
        m = np.zeros((N, n_cp, 3))
        if td is not None:
            m[:] = np.asarray(td, dtype=np.float64).reshape((-1, n_cp, 3))
        block = pack_state(
            lay,
            base_position=p,
            base_quaternion=q,
            joint_positions=s,
            base_linear_velocity=W_v[:, :3],
            base_angular_velocity=W_v[:, 3:],
            joint_velocities=sd,
            tangential_deformation=m,
            dtype=np.dtype(dtype),
        )
        tile = runtime.device_model(model, dtype).layout.tile
        return JaxSimModelData(model, runtime.DeviceArray.from_host(block, tile=tile), velocity_representation, batched)

    @staticmethod
    def zero(model, velocity_representation: VelRepr = VelRepr.Mixed, **kwargs) -> "JaxSimModelData":
        """``JaxSimModelData.zero`` (``src/jaxsim/api/data.py:204-222``)."""
        return JaxSimModelData.build(model, velocity_representation=velocity_representation, **kwargs)

    @staticmethod
    def from_state_block(model, block: np.ndarray, velocity_representation=VelRepr.Mixed) -> "JaxSimModelData":
        """Wrap a host ``[rows, N]`` block (inertial-fixed base velocity) -- no conversion."""
        lay = StateLayout.of(model)
        if block.shape[0] != lay.n_rows:
            raise ValueError((block.shape, lay.n_rows))
        tile = runtime.device_model(model, block.dtype).layout.tile
        return JaxSimModelData(model, runtime.DeviceArray.from_host(block, tile=tile), velocity_representation, True)

    # -- host views ---------------------------------------------------------------------------
    @property
    def dtype(self):
        return self._state.dtype

    @property
    def batch_size(self) -> int:
        return self._state.cols

    def state_block(self) -> np.ndarray:
        """Download the raw ``[rows, N]`` block."""
        return self._state.to_host()

    def _invalidate_caches(self) -> None:
        """The device buffer was overwritten (``step(..., inplace=True)``): forget the host copies."""
        self._host = None
        self._kin = None
        self._cent = None
        self._frames = None

    def _fields(self) -> dict:
        if self._host is None:
            self._host = unpack_state(StateLayout.of(self._model_ref), self._state.to_host())
        return self._host

    def _out(self, a: np.ndarray) -> np.ndarray:
        return a if self._batched else a[0]

    @property
    def joint_positions(self):
        return self._out(self._fields()["joint_positions"])

    @property
    def joint_velocities(self):
        return self._out(self._fields()["joint_velocities"])

    @property
    def base_position(self):
        return self._out(self._fields()["base_position"])

    @property
    def base_quaternion(self):
        return self._out(self._fields()["base_quaternion"])

    @property
    def base_orientation(self):
        """Normalised quaternion (``src/jaxsim/api/data.py:267-286``)."""
        q = self._fields()["base_quaternion"]
        norm = np.linalg.norm(q, axis=-1, keepdims=True)
        return self._out(q / (norm + np.finfo(q.dtype).eps * (norm == 0)))

    @property
    def _base_linear_velocity(self):
        return self._out(self._fields()["base_linear_velocity"])

    @property
    def _base_angular_velocity(self):
        return self._out(self._fields()["base_angular_velocity"])

    @property
    def contact_state(self) -> dict:
        return {"tangential_deformation": self._out(self._fields()["tangential_deformation"])}

    def _base_transform_batched(self) -> np.ndarray:
        f = self._fields()
        q = f["base_quaternion"].astype(np.float64)
        H = np.zeros((q.shape[0], 4, 4))
        H[:, :3, :3] = hm.quaternion_to_rotation(q / np.linalg.norm(q, axis=-1, keepdims=True))
        H[:, :3, 3] = f["base_position"]
        H[:, 3, 3] = 1
        return H

    @property
    def base_transform(self):
        return self._out(self._base_transform_batched().astype(self.dtype))

    @property
    def _base_transform(self):
        return self.base_transform

    def _base_velocity_batched(self, rep=None) -> np.ndarray:
        f = self._fields()
        W_v = np.concatenate([f["base_linear_velocity"], f["base_angular_velocity"]], -1).astype(np.float64)
        rep = self.velocity_representation if rep is None else rep
        return _inertial_to_other(W_v, rep, self._base_transform_batched(), False)

    @property
    def base_velocity(self):
        """Base 6D velocity in the active representation (``src/jaxsim/api/data.py:288-312``)."""
        return self._out(self._base_velocity_batched().astype(self.dtype))

    @property
    def generalized_velocity(self):
        v = np.concatenate([self._base_velocity_batched(), self._fields()["joint_velocities"]], -1)
        return self._out(v.astype(self.dtype))

    @property
    def generalized_position(self):
        return self.base_transform, self.joint_positions

    @contextlib.contextmanager
    def switch_velocity_representation(self, velocity_representation: VelRepr):
        """``switch_velocity_representation`` (``src/jaxsim/api/common.py:60-98``)."""
        old = self.velocity_representation
        self.velocity_representation = VelRepr(velocity_representation)
        try:
            yield self
        finally:
            self.velocity_representation = old

    # -- cached kinematics (computed by the MODE_KIN kernel on first use) -----------------------
    def _kinematics(self):
        if self._kin is None:
            model = self._model_ref
            dm = runtime.device_model(model, self.dtype)
            nL, N = model.number_of_links(), self.batch_size
            H = runtime.DeviceArray(nL * 12, N, self.dtype, tile=self._state.tile)
            V = runtime.DeviceArray(nL * 6, N, self.dtype, tile=self._state.tile)
            _lib.check(
                _lib.load().jxs_refresh_kinematics(
                    dm.handle, C.c_void_p(self._state.ptr), C.c_void_p(H.ptr), C.c_void_p(V.ptr), N, runtime._sp()
                ),
                "jxs_refresh_kinematics",
            )
            Hh = H.to_host().T.reshape(N, nL, 3, 4)
            full = np.zeros((N, nL, 4, 4), dtype=self.dtype)
            full[:, :, :3, :] = Hh
            full[:, :, 3, 3] = 1
            self._kin = (full, V.to_host().T.reshape(N, nL, 6).copy())
        return self._kin

    @property
    def _link_transforms(self):
        return self._out(self._kinematics()[0])

    @property
    def _link_velocities(self):
        return self._out(self._kinematics()[1])

    # -- functional update ----------------------------------------------------------------------
    def replace(
        self,
        model,
        joint_positions=None,
        joint_velocities=None,
        base_quaternion=None,
        base_linear_velocity=None,
        base_angular_velocity=None,
        base_position=None,
        *,
        contact_state: dict | None = None,
        validate: bool = False,
    ) -> "JaxSimModelData":
        """``JaxSimModelData.replace`` (``src/jaxsim/api/data.py:405-523``): the quaternion is
        re-normalised; base velocities, when given, are in the active representation."""
        f = self._fields()
        N = self.batch_size

        def pick(new, old):
            if new is None:
                return old
            a = np.asarray(new, dtype=np.float64)
            if old.size == 0:  # (a model without joints: the empty joint arrays of the reference)
                return old
            return np.broadcast_to(a.reshape((-1,) + old.shape[1:]), old.shape).copy()

        q = pick(base_quaternion, f["base_quaternion"]).astype(np.float64)
        nrm = np.linalg.norm(q, axis=-1, keepdims=True)
        q = q / np.where(nrm == 0, 1.0, nrm)
        p = pick(base_position, f["base_position"])
        vl, va = f["base_linear_velocity"], f["base_angular_velocity"]
        if base_linear_velocity is not None or base_angular_velocity is not None:
            act = self._base_velocity_batched()
            lin = pick(base_linear_velocity, act[:, :3])
            ang = pick(base_angular_velocity, act[:, 3:])
            H = np.zeros((N, 4, 4))
            H[:, :3, :3] = hm.quaternion_to_rotation(q)
            H[:, :3, 3] = p
            H[:, 3, 3] = 1
            W_v = _other_to_inertial(np.concatenate([lin, ang], -1), self.velocity_representation, H, False)
            vl, va = W_v[:, :3], W_v[:, 3:]
        m = f["tangential_deformation"]
        if contact_state is not None and "tangential_deformation" in contact_state:
            m = pick(contact_state["tangential_deformation"], m)
        block = pack_state(
            StateLayout.of(model),
            base_position=p,
            base_quaternion=q,
            joint_positions=pick(joint_positions, f["joint_positions"]),
            base_linear_velocity=vl,
            base_angular_velocity=va,
            joint_velocities=pick(joint_velocities, f["joint_velocities"]),
            tangential_deformation=m,
            dtype=self.dtype,
        )
        return JaxSimModelData(
            model, runtime.DeviceArray.from_host(block, tile=self._state.tile), self.velocity_representation, self._batched
        )

    def valid(self, model) -> bool:
        """Shape compatibility check (``src/jaxsim/api/data.py:525-549``)."""
        return self._state.rows == StateLayout.of(model).n_rows

    def copy(self) -> "JaxSimModelData":
        return JaxSimModelData(self._model_ref, self._state.copy(), self.velocity_representation, self._batched)

    # -- the episode loop around `step`: resets, gathers, scatters and flags that stay on the device ------------
    def _check_peer(self, other, what: str, *, same_batch: bool) -> None:
        """``other`` must hold states of the same model (the same state layout) in the same dtype -- and, for a
        ``same_batch`` operation, as many environments in the same tiling."""
        if not isinstance(other, JaxSimModelData):
            raise ValueError(f"{what} must be a JaxSimModelData, not {type(other).__name__}")
        if other._model_ref is not self._model_ref and (
            StateLayout.of(other._model_ref) != StateLayout.of(self._model_ref) or other._state.rows != self._state.rows
        ):
            raise ValueError(f"{what} belongs to another model (state rows {other._state.rows} != {self._state.rows})")
        if other.dtype != self.dtype:
            raise ValueError(f"{what} has dtype {other.dtype}, not {self.dtype}")
        if same_batch and (other.batch_size != self.batch_size or other._state.tile != self._state.tile):
            raise ValueError(
                f"{what} holds {other.batch_size} environments (tile {other._state.tile}), not {self.batch_size} (tile {self._state.tile})")

    def _check_spec(self, spec, cls, what: str) -> None:
        """The argument ``what`` must be a ``cls`` (``RandomStateDistribution``, or a spec of ``env_specs``: observation, action,
        reward, contact sensors) that was built for this object's model layout and dtype."""
        if not isinstance(spec, cls):
            raise ValueError(f"{what} must be {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__}, not {type(spec).__name__}")
        if spec.layout != StateLayout.of(self._model_ref) or spec.layout.n_rows != self._state.rows:
            raise ValueError(f"{what} was built for another model layout ({spec.layout} != {StateLayout.of(self._model_ref)})")
        if spec.dtype != self.dtype:
            raise ValueError(f"{what} was built for dtype {spec.dtype}, not {self.dtype}")

    def _check_block(self, name: str, blk, rows: int) -> None:
        """The argument ``name`` must be a tiled ``[rows][batch_size]`` ``DeviceArray`` of this object's dtype and tile."""
        st = self._state
        if not isinstance(blk, runtime.DeviceArray):
            raise ValueError(f"{name} must be a runtime.DeviceArray, not {type(blk).__name__}")
        if blk.shape != (rows, st.cols) or blk.dtype != st.dtype or blk.tile != st.tile:
            raise ValueError(f"{name} is {blk.shape} {blk.dtype} tile {blk.tile}: expected ({rows}, {st.cols}) {st.dtype} tile {st.tile}")

    def _matrix_arg(self, name: str, m, width: int, *, writable: bool):
        """``(device pointer, leading dimension, dtype)`` of the argument ``name``, an environment-major ``(batch_size, width)``
        matrix of float32 or this object's dtype: a ``runtime.DeviceMatrix`` or an object with a 2-D
        ``__cuda_array_interface__``, used in place.  ``None`` for anything else."""
        N, dt = self._state.cols, self.dtype
        if isinstance(m, runtime.DeviceMatrix):
            if m.shape != (N, width) or m.dtype not in (np.dtype(np.float32), dt):
                raise ValueError(f"{name} is {m.shape} {m.dtype}: expected ({N}, {width}) float32 or {dt}")
            return m.ptr, width, m.dtype
        if hasattr(m, "__cuda_array_interface__"):
            return runtime.foreign_matrix(m, N, width, tuple({"<f4", dt.str}), writable=writable)
        return None

    def _result(self, out: runtime.DeviceArray, inplace: bool) -> "JaxSimModelData":
        """What an operation with an ``inplace`` switch returns: this object, whose buffer ``out`` is and whose cached host
        copies are stale now, or a new object around ``out``."""
        if inplace:
            self._invalidate_caches()
            return self
        return JaxSimModelData(self._model_ref, out, self.velocity_representation, self._batched)

    def reset_where(self, mask, fresh: "JaxSimModelData", *, inplace: bool = False) -> "JaxSimModelData":
        """Environments whose ``mask`` entry is true take ``fresh``'s state, the others keep theirs -- the reference's
        ``jax.tree.map(lambda a, b: jnp.where(done, a, b), fresh, data)`` under ``vmap``, as one kernel (``jxs_env_select``)
        on the current stream: no download, no synchronisation.

        ``mask``: a host bool array / sequence of ``batch_size`` entries (uploaded), a ``runtime.DeviceMask`` (for
        instance ``env_flags()``: any non-zero byte is true), or any object with a ``__cuda_array_interface__`` of shape
        ``(batch_size,)``, contiguous, typestr ``|b1`` or ``|u1``, which is read in place.  ``fresh`` must hold the
        same model, dtype, batch size and tiling (``ValueError`` otherwise).  The base velocity is stored
        inertial-fixed in both, so nothing is converted; the result keeps this object's velocity representation and
        batched flag.  ``inplace=True`` overwrites this object's buffer and returns ``self``."""
        self._check_peer(fresh, "fresh", same_batch=True)
        st = self._state
        keep, mptr = runtime.as_device_mask(mask, st.cols)
        out = st if inplace else runtime.DeviceArray.like(st)
        _lib.check(
            _lib.load().jxs_env_select(mptr, fresh._state.ptr, st.ptr, out.ptr, st.rows, st.cols, st.tile, _lib.dtype_code(st.dtype), runtime._sp()),
            "jxs_env_select",
        )
        del keep  # (a mask uploaded here goes back to the pool behind the launch, ordered by the stream)
        return self._result(out, inplace)

    def reset_random_where(self, mask, dist: "RandomStateDistribution", *, seed: int = 0, draw: int = 0, first_env: int = 0,
                           inplace: bool = False) -> "JaxSimModelData":
        """Environments whose ``mask`` entry is true take a freshly sampled state of ``dist``, the others keep theirs -- the
        reference's ``jnp.where(done, random_model_data(model, key=k), data)`` under ``vmap`` as one kernel
        (``jxs_env_randomize``) on the current stream, with no ``fresh`` block: no allocation, download or synchronisation.

        ``mask``: as for ``reset_where`` (host bools, a ``runtime.DeviceMask`` such as ``env_flags()``, or a
        ``__cuda_array_interface__`` of bytes); ``None`` means every environment.  The state of environment ``e`` is a
        function of ``(seed, draw, first_env + e)`` and the bounds alone -- not of the batch size, the mask or the tiling --
        so an episode loop passes a new ``draw`` per reset, and a shard of a larger batch passes the global index of its
        first environment as ``first_env`` and draws what the whole batch would.  ``dist`` must have been built for this
        model layout and dtype (``ValueError`` otherwise); the sampled base velocity is expressed in ``dist``'s velocity
        representation and stored inertial-fixed.  ``inplace=True`` overwrites this object's buffer and returns ``self``;
        otherwise the block is copied first."""
        from .api.model import _device_model_fast

        self._check_spec(dist, RandomStateDistribution, "dist")
        st = self._state
        seed, draw, first_env = int(seed), int(draw), int(first_env)
        if not (0 <= seed < 2**64 and 0 <= draw < 2**64):
            raise ValueError("seed and draw must fit 64 unsigned bits")
        if first_env < 0 or first_env + st.cols > 2**32:
            raise ValueError(f"first_env = {first_env} with {st.cols} environments: global environment indices must stay below 2^32")
        keep, mptr = (None, None) if mask is None else runtime.as_device_mask(mask, st.cols)
        dm = _device_model_fast(self._model_ref, self.dtype)
        out = st if inplace else st.copy()
        _lib.check(
            _lib.load().jxs_env_randomize(dm.handle, mptr, out.ptr, st.cols, dist.bounds_ptr, seed, draw, first_env,
                                          int(dist.velocity_representation), runtime._sp()),
            "jxs_env_randomize",
        )  # fmt: skip
        del keep
        return self._result(out, inplace)

    def take(self, indices) -> "JaxSimModelData":
        """A new data object of the ``K`` environments ``indices`` (``jax.tree.map(lambda x: x[indices], data)``), gathered
        on the device (``jxs_env_copy``).  Host indices are checked here (``ValueError`` when out of range); indices on
        the device (``runtime.DeviceIndices`` or a ``__cuda_array_interface__`` of typestr ``<i4``) are checked by the
        kernel, which skips an out-of-range entry: that environment of the result is zero."""
        st = self._state
        keep, iptr, K, host = runtime.as_device_indices(indices, st.cols, unique=False)
        out = runtime.DeviceArray(st.rows, K, st.dtype, tile=st.tile, zero=host is None or K % st.tile != 0)
        _lib.check(
            _lib.load().jxs_env_copy(
                C.c_void_p(st.ptr), st.cols, st.tile, C.c_void_p(iptr), C.c_void_p(out.ptr), K, out.tile, None, st.rows, K,
                _lib.dtype_code(st.dtype), runtime._sp()
            ),
            "jxs_env_copy",
        )
        del keep
        return JaxSimModelData(self._model_ref, out, self.velocity_representation, self._batched or K != 1)

    def put(self, indices, other: "JaxSimModelData", *, inplace: bool = False) -> "JaxSimModelData":
        """Environment ``k`` of ``other`` (``K = len(indices)`` environments) replaces environment ``indices[k]``
        (``jax.tree.map(lambda x, y: x.at[indices].set(y), data, other)``), scattered on the device.  Host indices are
        checked here: out of range or twice the same raises ``ValueError``.  For indices on the device the kernel's
        rule holds: an out-of-range entry is skipped, a destination named twice is left unspecified."""
        self._check_peer(other, "other", same_batch=False)
        st = self._state
        keep, iptr, K, _ = runtime.as_device_indices(indices, st.cols, unique=True)
        if other.batch_size != K:
            raise ValueError(f"other holds {other.batch_size} environments for {K} indices")
        out = st if inplace else st.copy()
        _lib.check(
            _lib.load().jxs_env_copy(
                C.c_void_p(other._state.ptr), K, other._state.tile, None, C.c_void_p(out.ptr), st.cols, st.tile, C.c_void_p(iptr),
                st.rows, K, _lib.dtype_code(st.dtype), runtime._sp()
            ),
            "jxs_env_copy",
        )
        del keep
        return self._result(out, inplace)

    def env_flags(self) -> runtime.DeviceMask:
        """One byte per environment, on the device (``jxs_env_flags``): bit 0 = some state entry is NaN or infinite,
        bit 1 = the base quaternion holds no NaN and is not of unit norm.  The result can be passed to ``reset_where``
        as it is (every flagged environment is reset)."""
        from .api.model import _device_model_fast  # (the look-up of `step`: no model signature per call of the hot loop)

        dm = _device_model_fast(self._model_ref, self.dtype)
        flags = runtime.DeviceMask(self.batch_size)
        _lib.check(_lib.load().jxs_env_flags(dm.handle, self._state.ptr, self.batch_size, flags.ptr, runtime._sp()), "jxs_env_flags")
        return flags

    def nonfinite_mask(self):
        """Bit 0 of ``env_flags()`` as a host bool array: which environments hold a NaN or an infinity."""
        return self._out((self.env_flags().to_host() & 1) != 0)

    def _source_blocks(self, spec, sources: dict | None):
        """The source blocks of a launch of ``observe`` or ``evaluate``: those that ``spec`` names, out of ``sources``, in source
        order.  ``ValueError`` for a missing, unknown or mis-shaped source.  (``ptr`` records the stream: read it at the launch.)"""
        sources = dict(sources or {})
        unknown = sorted(set(sources) - set(spec.source_names))
        if unknown:
            raise ValueError(f"sources {unknown} are not named by the spec (it names {list(spec.source_names)})")
        blocks = []
        for name, rows in zip(spec.source_names, spec.source_rows):
            blk = sources.get(name)
            if blk is None:
                raise ValueError(f"the spec reads the source {name!r}, which was not given")
            self._check_block(f"source {name!r}", blk, rows)
            blocks.append(blk)
        return blocks

    def _spec_repr(self, spec) -> int:
        """The representation of the base velocity in a launch: the spec's, or this object's at the call if that is ``None``."""
        return int(self.velocity_representation if spec.velocity_representation is None else spec.velocity_representation)

    def observe(self, spec: "ObservationSpec", out=None, sources: dict | None = None):
        """The input of a policy, an environment-major ``(batch_size, spec.size)`` matrix on the device, assembled by one
        kernel (``jxs_env_observe``) on the current stream -- what the reference's user writes as ``jnp.concatenate`` of
        ``data.joint_positions``, ``data.base_orientation``, ``data.base_velocity`` ... under ``vmap``: no download, no
        synchronisation.

        ``sources``: ``{name: DeviceArray}`` for every source the spec names, each ``[rows][batch_size]`` of this object's
        dtype and tile (what ``centroidal_quantities(out=)``, ``frame.kinematics(out=)``, ``gravity_compensation_torques``
        return, or last step's torques).  ``out=None`` returns a new ``runtime.DeviceMatrix`` of ``spec.out_dtype``; a
        ``DeviceMatrix`` or any object with a 2-D ``__cuda_array_interface__`` of shape ``(batch_size, spec.size)``, typestr
        float32 or this object's dtype and strides ``None`` or ``(ld * itemsize, itemsize)``, ``ld >= spec.size``, is
        written in place (zero copy; only the ``spec.size`` columns of each row) and returned.  The base velocity is
        expressed in ``spec.velocity_representation``, or in this object's representation at the call if that is ``None``.
        ``ValueError`` before any launch for a spec of another layout or dtype, a missing, unknown or mis-shaped source, a
        wrong ``out``."""
        from .api.model import _device_model_fast

        self._check_spec(spec, ObservationSpec, "spec")
        st = self._state
        blocks = self._source_blocks(spec, sources)
        N, D = st.cols, spec.size
        if out is None:
            out = runtime.DeviceMatrix(N, D, spec.out_dtype)
        where = self._matrix_arg("out", out, D, writable=True)
        if where is None:
            raise ValueError(f"out must be None, a runtime.DeviceMatrix or a 2-D __cuda_array_interface__ object, not {type(out).__name__}")
        optr, ld, odt = where
        dm = _device_model_fast(self._model_ref, self.dtype)
        ptrs = (C.c_void_p * 4)(*[b.ptr for b in blocks])
        _lib.check(
            _lib.load().jxs_env_observe(dm.handle, spec._table(dm), st.ptr, ptrs, N, self._spec_repr(spec), optr, _lib.dtype_code(odt), ld, runtime._sp()),
            "jxs_env_observe",
        )
        return out

    def _action_tensor(self, spec: "ActionSpec", actions):
        """``(object to keep alive until the launch is enqueued, device pointer or None, leading dimension, dtype)`` of the
        ``actions`` argument of ``act``; a host array is uploaded on the current stream."""
        N, A, dt = self._state.cols, spec.width, self.dtype
        if actions is None:
            if spec.reads_actions:
                raise ValueError("actions is None, and the spec names action columns")
            return None, None, A, np.dtype(np.float32)
        where = self._matrix_arg("actions", actions, A, writable=False)
        if where is not None:
            return (actions, *where)
        a = np.asarray(actions)
        if a.dtype not in (np.dtype(np.float32), dt):
            a = a.astype(dt)
        if a.shape == (A,) and not self._batched:
            a = a.reshape(1, A)
        if a.shape != (N, A):
            raise ValueError(f"actions of shape {a.shape}: expected ({N}, {A})")
        m = runtime.DeviceMatrix.from_host(a)
        return m, m.ptr, A, m.dtype

    def act(self, spec: "ActionSpec", actions, *, feed_forward=None, out=None) -> runtime.DeviceArray:
        """The joint torques of a policy's action, a tiled ``[n][batch_size]`` ``runtime.DeviceArray``, computed by one kernel
        (``jxs_env_act``) on the current stream from the action tensor and this object's joint positions and velocities -- the
        controller that the reference's user carries through a ``jax.lax.scan`` of ``step`` under ``vmap``: no download, no
        synchronisation.  The result goes straight into ``step(joint_force_references=...)``.

        ``actions``: a ``runtime.DeviceMatrix`` ``(batch_size, spec.width)``; any object with a 2-D
        ``__cuda_array_interface__`` of that shape, typestr float32 or this object's dtype and strides ``None`` or
        ``(ld * itemsize, itemsize)`` (read in place, zero copy); a host array of that shape (uploaded); ``None`` when the spec
        names no column.  ``feed_forward``: a ``DeviceArray`` ``[n][batch_size]`` of this object's dtype and tile added before
        the torque limit (what ``gravity_compensation_torques`` returns).  ``out``: such an array to write into.
        ``ValueError`` before any launch for a spec of another layout or dtype, a wrong ``actions`` shape or dtype, a
        mis-shaped ``feed_forward`` or ``out``."""
        from .api.model import _device_model_fast

        self._check_spec(spec, ActionSpec, "spec")
        st = self._state
        N, n = st.cols, spec.layout.n_joints
        for name, blk in (("feed_forward", feed_forward), ("out", out)):
            if blk is not None:
                self._check_block(name, blk, n)
        keep, aptr, ld, adt = self._action_tensor(spec, actions)
        if out is None:
            out = runtime.DeviceArray(n, N, st.dtype, tile=st.tile)
        dm = _device_model_fast(self._model_ref, self.dtype)
        _lib.check(
            _lib.load().jxs_env_act(dm.handle, spec._table(dm), st.ptr, aptr, _lib.dtype_code(adt), ld,
                                    None if feed_forward is None else feed_forward.ptr, out.ptr, N, runtime._sp()),
            "jxs_env_act",
        )  # fmt: skip
        del keep
        return out

    def evaluate(self, spec: "RewardSpec", *, sources: dict | None = None, reward=None, done=None, terms=None, fired=None, steps=None,
                 max_steps: int = 0):  # fmt: skip
        """``(reward, done)`` of a policy step, computed by one kernel (``jxs_env_evaluate``) on the current stream -- the reward
        function and the done predicate that the reference's user writes over ``data.base_position``, ``data.joint_positions``,
        ``data.base_velocity`` ... under ``vmap``: no download, no synchronisation.  ``done`` holds one byte per environment, bit 0
        ``DONE_TERMINATED``, bit 1 ``DONE_TRUNCATED``, and goes into ``reset_where`` / ``reset_random_where`` as it is.

        ``sources``: as for ``observe``, ``{name: DeviceArray}`` for every source the spec names (also as a target).
        ``reward=None`` returns a new ``runtime.DeviceMatrix`` ``(batch_size, 1)`` of this object's dtype; a ``DeviceMatrix`` of
        that shape or an object with a ``__cuda_array_interface__`` of shape ``(batch_size,)`` or ``(batch_size, 1)``, contiguous,
        float32 or this object's dtype, is written in place.  ``done=None`` returns a new ``runtime.DeviceMask``; a ``DeviceMask``
        or a ``__cuda_array_interface__`` of ``batch_size`` bytes (``|u1`` / ``|b1``) is written in place.  Optional outputs,
        written only when given: ``fired``, a ``runtime.DeviceWords`` or ``<u4`` device vector (bit ``c``: condition
        ``spec.condition_names[c]`` fired); ``terms``, a ``DeviceMatrix`` or 2-D ``__cuda_array_interface__`` ``(batch_size,
        spec.n_terms)`` with a row stride, float32 or this object's dtype (column ``t``: the contribution of
        ``spec.term_names[t]``).  ``steps``: the episode counters, a ``runtime.DeviceIndices`` or ``<i4`` device vector, updated in
        place with ``max_steps > 0``: an environment whose counter reaches ``max_steps`` is truncated, and the counter of every
        environment flagged done restarts at zero.  ``ValueError`` before any launch for a spec of another layout or dtype, a
        missing, unknown or mis-shaped source, a wrong output, ``steps`` without a positive ``max_steps``."""
        from .api.model import _device_model_fast

        self._check_spec(spec, RewardSpec, "spec")
        st = self._state
        blocks = self._source_blocks(spec, sources)
        N, K, dt = st.cols, spec.n_terms, self.dtype
        floats = tuple({"<f4", dt.str})

        def vector(name, v, cls, typestrs):
            """The device pointer of an optional integer output: a ``cls`` or a foreign 1-D vector of ``N`` entries."""
            if isinstance(v, cls):
                if v.n != N:
                    raise ValueError(f"{name} of {v.n} entries: expected {N}")
                return v.ptr
            if not isinstance(v, runtime._DeviceVector) and hasattr(v, "__cuda_array_interface__"):
                return runtime.foreign_vector(v, N, typestrs)[0]
            raise ValueError(f"{name} must be a runtime.{cls.__name__} or a __cuda_array_interface__ object of typestr {typestrs}, not {type(v).__name__}")

        if reward is None:
            reward = runtime.DeviceMatrix(N, 1, dt)
        if hasattr(reward, "__cuda_array_interface__") and not isinstance(reward, runtime.DeviceMatrix) and len(reward.__cuda_array_interface__["shape"]) == 1:
            rptr, rdt = runtime.foreign_vector(reward, N, floats)[0], np.dtype(reward.__cuda_array_interface__["typestr"])
        else:
            where = self._matrix_arg("reward", reward, 1, writable=True)
            if where is None:
                raise ValueError(f"reward must be None, a runtime.DeviceMatrix or a __cuda_array_interface__ object, not {type(reward).__name__}")
            rptr, ld, rdt = where
            if ld != 1 and N > 1:
                raise ValueError("reward must be contiguous")
        if done is None:
            done = runtime.DeviceMask(N)
        dptr = vector("done", done, runtime.DeviceMask, runtime.MASK_TYPESTRS)
        fptr = None if fired is None else vector("fired", fired, runtime.DeviceWords, ("<u4",))
        sptr = None if steps is None else vector("steps", steps, runtime.DeviceIndices, runtime.INDEX_TYPESTRS)
        max_steps = int(max_steps)
        if steps is not None and max_steps <= 0:
            raise ValueError(f"steps is given, and max_steps = {max_steps} is not positive")
        tptr, tld, tdt = None, K, dt
        if terms is not None:
            if K == 0:
                raise ValueError("terms is given, and the spec has no reward term")
            where = self._matrix_arg("terms", terms, K, writable=True)
            if where is None:
                raise ValueError(f"terms must be a runtime.DeviceMatrix or a 2-D __cuda_array_interface__ object, not {type(terms).__name__}")
            tptr, tld, tdt = where
        dm = _device_model_fast(self._model_ref, self.dtype)
        ptrs = (C.c_void_p * 4)(*[b.ptr for b in blocks])
        _lib.check(
            _lib.load().jxs_env_evaluate(dm.handle, spec._table(dm), st.ptr, ptrs, N, self._spec_repr(spec), rptr, _lib.dtype_code(rdt), dptr, fptr, tptr,
                                         _lib.dtype_code(tdt), tld, sptr, max_steps, runtime._sp()),
            "jxs_env_evaluate",
        )  # fmt: skip
        return reward, done

    def link_kinematics(self, out=None):
        """``(link_transforms, link_velocities)`` of ``jxs_refresh_kinematics`` as they are on the device: two tiled
        ``DeviceArray``s ``[nL*12][batch_size]`` (rows of ``[R|p]`` per link) and ``[nL*6][batch_size]`` (inertial-fixed link
        velocities), one launch on the current stream, no download -- what ``contact_sensors`` reads.  ``out``: a pair of
        blocks of these shapes to write into."""
        from . import specialize
        from .api.model import _device_model_fast

        st, nL = self._state, self._model_ref.number_of_links()
        if out is None:
            out = (runtime.DeviceArray(nL * 12, st.cols, st.dtype, tile=st.tile), runtime.DeviceArray(nL * 6, st.cols, st.dtype, tile=st.tile))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be None or a pair (link_transforms, link_velocities) of runtime.DeviceArray")
        H, V = out
        self._check_block("out[0] (link_transforms)", H, nL * 12)
        self._check_block("out[1] (link_velocities)", V, nL * 6)
        dm = _device_model_fast(self._model_ref, self.dtype)
        specialize.ensure_mode(dm, self._model_ref, specialize.MODE_KIN)  # (first call: cached object, or built when hipcc is there)
        _lib.check(_lib.load().jxs_refresh_kinematics(dm.handle, C.c_void_p(st.ptr), C.c_void_p(H.ptr), C.c_void_p(V.ptr), st.cols, runtime._sp()),
                   "jxs_refresh_kinematics")  # fmt: skip
        return H, V

    def contact_sensors(self, spec: "ContactSensorSpec", *, kinematics=None, timers=None, reset=None, dt=None, out=None) -> runtime.DeviceArray:
        """The contact record of ``spec``, a tiled ``DeviceArray`` ``[spec.n_rows][batch_size]`` written by one kernel
        (``jxs_env_contacts``) on the current stream: per group of points the rows ``CONTACT_FIELDS`` -- contact flag, number
        of points in contact, smallest clearance, largest squared slip speed of the points in contact, air time, contact
        time, touchdown and the length of the flight that just ended --, what the reference's user derives from
        ``js.contact.in_contact`` and ``js.contact.collidable_point_kinematics`` under ``vmap``.  The record is a source block
        of ``observe`` and ``evaluate`` (``spec.source``): no download, no synchronisation.

        ``kinematics``: the pair ``link_kinematics()`` returned for this state (``None``: computed here, one more launch), or
        the transforms alone, ``(link_transforms, None)``: no slip.  ``timers``: the in/out block of ``spec.new_timers``
        (``None``: rows 4-7 are zero and nothing is carried).  ``reset``: what ``reset_where`` takes as a mask, the ``done``
        of ``evaluate`` included: those environments start from zero timers.  ``dt``: the time a call stands for (default:
        the model's time step).  ``out``: a block to write into.  ``ValueError`` before any launch for a spec of another
        model or dtype or a mis-shaped block."""
        from .api.model import _device_model_fast

        self._check_spec(spec, ContactSensorSpec, "spec")
        st, nL = self._state, self._model_ref.number_of_links()
        if spec.n_links != nL:
            raise ValueError(f"spec was built for a model of {spec.n_links} links, not {nL}")
        if kinematics is None:
            kinematics = self.link_kinematics()
        if not isinstance(kinematics, (tuple, list)) or len(kinematics) != 2:
            raise ValueError("kinematics must be None or the pair (link_transforms, link_velocities) of link_kinematics()")
        H, V = kinematics
        self._check_block("kinematics[0] (link_transforms)", H, nL * 12)
        if V is not None:
            self._check_block("kinematics[1] (link_velocities)", V, nL * 6)
        if timers is not None:
            self._check_block("timers", timers, spec.n_timer_rows)
        if out is None:
            out = runtime.DeviceArray(spec.n_rows, st.cols, st.dtype, tile=st.tile)
        self._check_block("out", out, spec.n_rows)
        dt = float(self._model_ref.time_step if dt is None else dt)
        if not (np.isfinite(dt) and dt >= 0.0):
            raise ValueError(f"dt = {dt} must be finite and not negative")
        keep, mptr = (None, None) if reset is None else runtime.as_device_mask(reset, st.cols)
        dm = _device_model_fast(self._model_ref, self.dtype)
        _lib.check(
            _lib.load().jxs_env_contacts(dm.handle, spec._table(dm), C.c_void_p(H.ptr), None if V is None else C.c_void_p(V.ptr), st.cols, dt, mptr,
                                         None if timers is None else C.c_void_p(timers.ptr), C.c_void_p(out.ptr), runtime._sp()),
            "jxs_env_contacts",
        )  # fmt: skip
        del keep
        return out


def random_model_data(
    model,
    *,
    batch_size: int = 1,
    seed: int = 0,
    velocity_representation: VelRepr = VelRepr.Mixed,
    base_pos_bounds=((-1, -1, 0.5), (1, 1, 1)),
    base_rpy_bounds=((-np.pi,) * 3, (np.pi,) * 3),
    base_vel_lin_bounds=((-1,) * 3, (1,) * 3),
    base_vel_ang_bounds=((-1,) * 3, (1,) * 3),
    joint_vel_bounds=(-1.0, 1.0),
    dtype=np.float64,
) -> JaxSimModelData:
    """Same distribution as the reference's ``random_model_data``
    (``src/jaxsim/api/data.py:552-682``) drawn from NumPy's PCG64 -- JAX's threefry stream
    cannot be reproduced bit-exactly and need not be."""
    rng = np.random.default_rng(seed)
    kdp = model.kin_dyn_parameters
    N, n = batch_size, kdp.number_of_joints()
    p = rng.uniform(*np.array(base_pos_bounds, dtype=float), size=(N, 3))
    q = hm.rpy_to_quaternion(rng.uniform(*np.array(base_rpy_bounds, dtype=float), size=(N, 3)))
    lo = np.maximum(kdp.position_limits_min, -10.0)
    hi = np.minimum(kdp.position_limits_max, 10.0)
    s = rng.uniform(lo, hi, size=(N, n)) if n else np.zeros((N, 0))
    sd = rng.uniform(*joint_vel_bounds, size=(N, n)) if n else np.zeros((N, 0))
    vl = rng.uniform(*np.array(base_vel_lin_bounds, dtype=float), size=(N, 3))
    va = rng.uniform(*np.array(base_vel_ang_bounds, dtype=float), size=(N, 3))
    if not model.floating_base():
        vl, va = np.zeros_like(vl), np.zeros_like(va)
    return JaxSimModelData.build(
        model,
        base_position=p,
        base_quaternion=q,
        joint_positions=s,
        base_linear_velocity=vl,
        base_angular_velocity=va,
        joint_velocities=sd,
        velocity_representation=velocity_representation,
        batch_size=N,
        dtype=dtype,
    )


def _bounds_pair(bounds, width: int, what: str) -> np.ndarray:
    """``(lo, hi)``, each a scalar or a sequence of ``width`` entries, as a ``[2, width]`` float64 array."""
    if len(bounds) != 2:
        raise ValueError(f"{what} must be a pair (lower, upper)")
    out = np.empty((2, width))
    for k in range(2):
        a = np.asarray(bounds[k], dtype=float)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, width)):
            raise ValueError(f"{what}[{k}] of shape {a.shape}: expected a scalar or {width} entries")
        out[k] = a
    return out


def random_state_bounds(
    model,
    *,
    dtype=np.float32,
    base_pos_bounds=((-1, -1, 0.5), 1.0),
    base_rpy_bounds=(-np.pi, np.pi),
    joint_pos_bounds=None,
    base_vel_lin_bounds=(-1.0, 1.0),
    base_vel_ang_bounds=(-1.0, 1.0),
    joint_vel_bounds=(-1.0, 1.0),
) -> np.ndarray:
    """The host bounds table ``[2][12 + 2n]`` of ``jxs_env_randomize`` (row of lower, row of upper bounds, rounded to
    ``dtype``) from the arguments of the reference's ``random_model_data`` (``src/jaxsim/api/data.py:552-586``: the same
    defaults, each bound a scalar or one value per component).  Variables: 3 base position, 3 XYZ Euler angles, n joint
    positions, 3 linear and 3 angular base velocity, n joint velocities.  ``joint_pos_bounds=None``: the joint limits by
    the rule of ``js.joint.random_joint_positions``.  ``ValueError`` for a bound that is not finite in ``dtype`` or
    lies above its partner."""
    from .api import joint as _joint

    n = model.kin_dyn_parameters.number_of_joints()
    dt = np.dtype(dtype)
    _lib.dtype_code(dt)
    if joint_pos_bounds is None:
        s = np.stack(_joint.random_position_bounds(model, dtype=dt)).astype(float) if n else np.empty((2, 0))
    else:
        s = _bounds_pair(joint_pos_bounds, n, "joint_pos_bounds")
    table = np.concatenate(
        [
            _bounds_pair(base_pos_bounds, 3, "base_pos_bounds"),
            _bounds_pair(base_rpy_bounds, 3, "base_rpy_bounds"),
            s,
            _bounds_pair(base_vel_lin_bounds, 3, "base_vel_lin_bounds"),
            _bounds_pair(base_vel_ang_bounds, 3, "base_vel_ang_bounds"),
            _bounds_pair(joint_vel_bounds, n, "joint_vel_bounds"),
        ],
        axis=1,
    )
    with np.errstate(over="ignore", invalid="ignore"):
        table = table.astype(dt)
        finite = np.isfinite(table).all(axis=0) & np.isfinite(table[1] - table[0])
    if not finite.all():
        raise ValueError(f"bounds of the variables {np.nonzero(~finite)[0].tolist()} are not finite in {dt.name}: "
                         "pass explicit finite bounds (joint_pos_bounds for joints without position limits)")
    if (table[0] > table[1]).any():
        raise ValueError(f"lower bound above upper bound for the variables {np.nonzero(table[0] > table[1])[0].tolist()}")
    return np.ascontiguousarray(table)


class RandomStateDistribution:
    """The uniform distribution of reset states of one model, with its bounds table resident on the device: what
    ``JaxSimModelData.reset_random_where`` and ``random_model_data_device`` sample from.  Built once (one small upload),
    used for every reset of an episode loop."""

    def __init__(self, layout: StateLayout, dtype, velocity_representation: VelRepr, bounds_host: np.ndarray):
        self.layout = layout
        self.dtype = np.dtype(dtype)
        self.velocity_representation = VelRepr(velocity_representation)
        self.bounds_host = bounds_host  # [2, 12 + 2n], in `dtype`
        self._bounds = runtime.DeviceArray(1, bounds_host.size, self.dtype, tile=1)  # (flat: one row, environment-major)
        _lib.check(
            _lib.load().jxs_memcpy_h2d(C.c_void_p(self._bounds.ptr), bounds_host.ctypes.data_as(C.c_void_p), bounds_host.nbytes, runtime._sp()),
            "jxs_memcpy_h2d",
        )
        # the one-off upload is waited for here: the table may be read by a reset on ANY stream afterwards
        # (runtime.set_stream between build and use), and nothing else would order that stream behind this copy
        runtime.synchronize()

    @property
    def bounds_ptr(self):
        return self._bounds.ptr

    @staticmethod
    def build(model, *, dtype=np.float32, velocity_representation: VelRepr = VelRepr.Mixed, **bounds) -> "RandomStateDistribution":
        """``bounds``: ``base_pos_bounds``, ``base_rpy_bounds``, ``joint_pos_bounds``, ``base_vel_lin_bounds``,
        ``base_vel_ang_bounds``, ``joint_vel_bounds`` as for ``random_state_bounds`` (the reference's defaults)."""
        runtime.require_device()
        table = random_state_bounds(model, dtype=dtype, **bounds)
        return RandomStateDistribution(StateLayout.of(model), dtype, velocity_representation, table)


def random_model_data_device(
    model,
    *,
    batch_size: int,
    dist: RandomStateDistribution | None = None,
    seed: int = 0,
    draw: int = 0,
    first_env: int = 0,
    dtype=np.float32,
    **bounds,
) -> JaxSimModelData:
    """A new batch of ``batch_size`` random states filled entirely on the device (``jxs_env_randomize`` over every
    environment): no host sampling, packing or upload.  ``dist``: a ``RandomStateDistribution`` to reuse; otherwise one is
    built from ``dtype`` and ``bounds`` (``velocity_representation`` and the bounds of ``random_state_bounds``).  The state
    of environment ``e`` is the one ``reset_random_where`` gives it for the same ``(seed, draw, first_env)``.  The host
    ``random_model_data`` (NumPy's PCG64) is a different stream."""
    if dist is None:
        dist = RandomStateDistribution.build(model, dtype=dtype, **bounds)
    elif bounds:
        raise ValueError(f"pass either dist or bounds, not both ({sorted(bounds)})")
    if int(batch_size) <= 0:
        raise ValueError("batch_size must be positive")
    tile = runtime.device_model(model, dist.dtype).layout.tile
    state = runtime.DeviceArray(dist.layout.n_rows, int(batch_size), dist.dtype, tile=tile, zero=int(batch_size) % tile != 0)
    data = JaxSimModelData(model, state, dist.velocity_representation, True)
    return data.reset_random_where(None, dist, seed=seed, draw=draw, first_env=first_env, inplace=True)
