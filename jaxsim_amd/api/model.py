"""``jaxsim.api.model`` mirror for the hot path: the Python functions a jaxsim user calls.

Every function launches the HIP kernels through the C-ABI; there is no CPU fallback.
Representation handling at the boundary (Inertial / Body / Mixed, default Mixed on the data
object) follows the reference wrappers and is done in NumPy on the few [N,6] base
quantities; the batched state itself never leaves the GPU inside ``step``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, runtime
from ..data import JaxSimModelData, _inertial_to_other, _other_to_inertial
from ..model import JaxSimModel, VelRepr  # noqa: F401
from ..runtime import DeviceArray


def _as_device(x, rows: int, N: int, dtype, trailing_shape, tile: int) -> DeviceArray | None:
    """Accept None | DeviceArray ([rows][N]) | an object with ``__cuda_array_interface__`` holding a
    contiguous device array ``[N, *trailing]`` | host array ([N, *trailing] or [*trailing])."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        if x.shape != (rows, N) or x.dtype != np.dtype(dtype):
            raise ValueError((x.shape, (rows, N)))
        return x
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is not None:
        # a device array of another framework (DLPack / CUDA array interface): contiguous [N, *trailing]
        # of the data's dtype; tiled on the device, no host round trip
        if tuple(cai["shape"]) != (N,) + tuple(trailing_shape) or np.dtype(cai["typestr"]) != np.dtype(dtype):
            raise ValueError((tuple(cai["shape"]), cai["typestr"], (N,) + tuple(trailing_shape), np.dtype(dtype).str))
        if cai.get("strides") is not None:
            raise ValueError("device arrays must be C-contiguous")
        return DeviceArray.from_device_env_major(cai["data"][0], N, rows, dtype, tile=tile)
    a = np.asarray(x, dtype=np.float64)
    a = a.squeeze() if a.ndim > len(trailing_shape) + 1 else a
    if a.shape == tuple(trailing_shape):
        a = np.broadcast_to(a, (N,) + tuple(trailing_shape))
    if a.shape != (N,) + tuple(trailing_shape):
        raise ValueError((a.shape, (N,) + tuple(trailing_shape)))  # cf. rbda/utils.py:102-133
    return DeviceArray.from_host(np.ascontiguousarray(a.reshape(N, rows).T), tile=tile, dtype=dtype)


_environ = __import__("os").environ
# os.environ.get() encodes its key and decodes the value on every call (1.1 us each -- a sixth of a step at 1024
# environments); the mapping underneath holds both as bytes and is what os.environ[...] = ... / monkeypatch.setenv write
_env_raw = getattr(_environ, "_data", None)
if _env_raw is not None and not (isinstance(_env_raw, dict) and isinstance(_environ.encodekey("X"), bytes) and isinstance(_environ.encodevalue("1"), bytes)):
    _env_raw = None  # (a platform whose os.environ keeps str underneath: the bytes comparisons below would never match)
_K_EXC, _K_SPEC = (_environ.encodekey("JAXSIM_ENABLE_EXCEPTIONS"), _environ.encodekey("JAXSIM_AMD_SPECIALIZE")) if _env_raw is not None else (None, None)
_TRUE = (b"1", b"true", b"on", b"yes")


def _exceptions_enabled() -> bool:
    """``JAXSIM_ENABLE_EXCEPTIONS`` (``src/jaxsim/exceptions.py:26-29``), same variable, same default."""
    if _env_raw is not None:
        v = _env_raw.get(_K_EXC)
        return v is not None and v.lower() in _TRUE
    v = _environ.get("JAXSIM_ENABLE_EXCEPTIONS")
    return v is not None and v.lower() in ("1", "true", "on", "yes")


def _policy_token():
    """The raw value of JAXSIM_AMD_SPECIALIZE (the kernel policy is part of what a cached device model was made under)."""
    return _env_raw.get(_K_SPEC) if _env_raw is not None else _environ.get("JAXSIM_AMD_SPECIALIZE")


def _device_model_fast(model, dtype):
    """``runtime.device_model`` without recomputing the model signature on every call of the hot loop.

    A `JaxSimModel` drops its cached device copies whenever one of its fields is assigned (``model.__setattr__``,
    ``editable()``), its sub-objects are frozen dataclasses, and the kernel policy is an environment variable: so the
    record ``(policy value, device model)`` kept NEXT to the device copies is valid while it is there and the variable
    has the value it was made under -- two dictionary look-ups instead of a 25-field tuple compare per step."""
    dev = model.__dict__.get("_device")
    key = ("fast", dtype.str)
    if dev is not None:
        rec = dev.get(key)
        if rec is not None and rec[0] == _policy_token():
            return rec[1]
    dm = runtime.device_model(model, dtype)
    model.__dict__.setdefault("_device", {})[key] = (_policy_token(), dm)
    return dm


def _check_quaternion(model, data: JaxSimModelData, *, normalized: bool) -> None:
    """The value checks of ``rbda/utils.py:135-146`` on the device state (only when exceptions are on)."""
    if not _exceptions_enabled():
        return
    dm = runtime.device_model(model, data.dtype)
    counts = (C.c_int * 3)()
    _lib.check(
        _lib.load().jxs_validate_state(dm.handle, C.c_void_p(data._state.ptr), data.batch_size, counts, runtime._sp()),
        "jxs_validate_state",
    )
    if counts[0]:
        raise ValueError("A RBDA received a quaternion that contains NaN values.")
    if normalized and counts[1]:
        raise ValueError("A RBDA received a quaternion that is not normalized.")


def solver_fault_counts(model: JaxSimModel, dtype=np.float64, *, reset: bool = False) -> tuple[int, int]:
    """RigidContacts / RelaxedRigidContacts: environments whose contact-force solve / impact solve was discarded
    (non-finite result) by the steps of this model since the last reset -- ``(contact_force_solves, impact_solves)``
    (the relaxed model has no impact: its second count stays 0).  The reference
    would carry the NaN into the state (``rbda/contacts/rigid.py:331-379``); here the environment takes that
    step without contact forces, and the event is counted instead of being silent."""
    dm = runtime.device_model(model, np.dtype(dtype))
    counts = (C.c_int * 2)()
    _lib.check(_lib.load().jxs_solver_fault_counts(dm.handle, counts, int(bool(reset)), runtime._sp()), "jxs_solver_fault_counts")
    return int(counts[0]), int(counts[1])


def _check_solver_faults(model, data: JaxSimModelData) -> None:
    """With ``JAXSIM_ENABLE_EXCEPTIONS`` a discarded solve raises like the reference's NaN checks would."""
    if not _exceptions_enabled() or type(model.contact_model).__name__ not in ("RigidContacts", "RelaxedRigidContacts"):
        return
    qp, imp = solver_fault_counts(model, data.dtype, reset=True)
    if qp or imp:
        raise ValueError(f"{type(model.contact_model).__name__}: {qp} contact-force solve(s) and {imp} impact solve(s) were not finite and were discarded")


def _ptr(d: DeviceArray | None):
    return None if d is None else C.c_void_p(d.ptr)


def reduce(model: JaxSimModel, considered_joints, locked_joint_positions: dict | None = None) -> JaxSimModel:
    """``js.model.reduce`` (``src/jaxsim/api/model.py:807-878``): lump the links connected by the
    joints that are not in ``considered_joints``, locked at ``locked_joint_positions`` (default 0).
    The reduced model keeps the time step, terrain, contact model / parameters, actuation parameters,
    gravity and integrator of ``model``."""
    src = model.__dict__.get("built_from")
    if src is None:
        raise ValueError("the model was not built from a model description: nothing to reduce")
    locked = dict(locked_joint_positions or {})
    return JaxSimModel.build_from_model_description(
        src,
        model_name=model.name(),
        time_step=model.time_step,
        terrain=model.terrain,
        contact_model=model.contact_model,
        contact_params=model.contact_params,
        actuation_params=model.actuation_params,
        integrator=model.integrator,
        gravity=-model.gravity,
        considered_joints=tuple(considered_joints),
        locked_joint_positions=locked,
    )


def specialize(model: JaxSimModel, dtype=np.float32, *, queries: bool = False) -> bool:
    """Build (hipcc, seconds) and attach the step / rollout kernels specialised on this model's kinematic tree --
    the counterpart of the reference compiling ``step`` per model under ``jax.jit`` (api/model.py:36-120 static
    fields).  Physical parameters stay run-time data.  ``queries=True`` does the same for the kernels behind
    ``forward_dynamics_aba``, ``inverse_dynamics``, the cached kinematics, the mass matrix, its inverse, the
    Jacobians and ``js.ode.system_dynamics``.  ``JAXSIM_AMD_SPECIALIZE=1`` specialises the step kernels of every model on first use."""
    from .. import specialize as _sp

    dm = runtime.device_model(model, np.dtype(dtype))
    done = _sp.attach(dm, model, build=True)
    if queries:
        done = _sp.attach(dm, model, _sp.QUERY_MODES + (_sp.dyn_mode_of(model),), build=True) or done
    return done


def step(
    model: JaxSimModel,
    data: JaxSimModelData,
    *,
    link_forces=None,
    joint_force_references=None,
    inplace: bool = False,
    gravity_compensation: bool = False,
) -> JaxSimModelData:
    """``js.model.step`` (``src/jaxsim/api/model.py:2601-2681``).

    ``gravity_compensation=True`` (extension): the joint part of ``free_floating_gravity_forces`` of ``data`` is added
    to ``joint_force_references`` -- what ``step(..., joint_force_references=gravity_compensation_torques(model, data) +
    tau)`` computes, in one launch for the rigid contact models (``jxs_step_gravity_compensated``) and as those two
    launches otherwise.

    ``link_forces`` ([N, nL, 6] or [nL, 6]) are expressed in ``data.velocity_representation``
    exactly like the reference (``:2641-2646``); ``joint_force_references`` is [N, n] or [n].
    Returns a new data object (functional); ``inplace=True`` (extension) updates ``data``'s
    buffer instead and returns a data object sharing it.
    """
    st = data._state
    dtype, N = st.dtype, st.cols
    dm = _device_model_fast(model, dtype)
    checks = _exceptions_enabled()  # (the reference's value checks are compiled in only with JAXSIM_ENABLE_EXCEPTIONS)
    if checks:
        _check_quaternion(model, data, normalized=False)  # ABA receives data.base_orientation (normalised)
    lib = _lib.load()
    stream = runtime._sp()
    if link_forces is None and joint_force_references is None and not gravity_compensation:
        # the reference's idiom `data = js.model.step(model, data)` (README.md:80-83, tests/test_simulations.py:170-191): no
        # inputs to convert -- pointers as plain integers (the C-ABI declares void*), the output block from the pool
        out = st if inplace else DeviceArray.like(st)
        rc = lib.jxs_step(dm.handle, st.ptr, out.ptr, None, None, int(data.velocity_representation), N, stream)
        if rc != 0:
            _lib.check(rc, "jxs_step")
    else:
        nL, n = model.number_of_links(), model.dofs()
        f = _as_device(link_forces, nL * 6, N, dtype, (nL, 6), st.tile)
        tau = _as_device(joint_force_references, n, N, dtype, (n,), st.tile)
        out = st if inplace else DeviceArray(st.rows, N, dtype, tile=st.tile)
        fn = lib.jxs_step
        if gravity_compensation:
            from .. import specialize as _sp

            if _sp.mode_of(model) in (_sp.MODE_STEP_RIGID, _sp.MODE_STEP_RK4_RIGID):
                fn = lib.jxs_step_gravity_compensated
            else:
                # soft contacts: g(q) through the host (no fused kernel for this mode), the user's references added to it
                # [ADVICE r4] -- whatever form they came in: a DeviceArray ([n][N]) and a device array of another
                # framework are downloaded, not handed to np.asarray
                g = np.asarray(free_floating_gravity_forces(model, data))[..., 6:]
                g = g.reshape(N, n) if g.ndim == 1 else g
                tau_np = g if tau is None else g + tau.to_host().T.astype(g.dtype)
                tau = _as_device(tau_np, n, N, dtype, (n,), st.tile)
        _lib.check(
            fn(dm.handle, C.c_void_p(st.ptr), C.c_void_p(out.ptr), _ptr(tau), _ptr(f), int(data.velocity_representation), N, stream),
            "jxs_step",
        )  # fmt: skip
    if checks:
        _check_solver_faults(model, data)
    if inplace:
        # the buffer of `data` now holds the new state: its lazily downloaded fields and cached
        # kinematics describe the old one
        data._invalidate_caches()
    return JaxSimModelData(model, out, data.velocity_representation, data._batched)


def control_steps(model: JaxSimModel, data: JaxSimModelData, spec, actions, n_substeps: int, *, feed_forward=None,
                  inplace: bool = True) -> JaxSimModelData:  # fmt: skip
    """``n_substeps`` physics steps under one policy action (extension): the decimation loop of a learning environment, two
    launches per sub-step -- ``data.act(spec, actions)`` reads the CURRENT joint positions and velocities and writes the
    torques, ``step`` consumes them -- so that the PD law runs at the physics rate.  Everything is enqueued on the current
    stream; nothing synchronises.  ``actions`` as for ``JaxSimModelData.act`` (a host array is uploaded once);
    ``feed_forward`` is the same block for every sub-step.  ``inplace=True`` advances ``data``'s buffer; ``inplace=False``
    leaves ``data`` untouched and returns a new object."""
    if int(n_substeps) < 1:
        raise ValueError("n_substeps must be at least 1")
    from ..data import ActionSpec

    if not isinstance(spec, ActionSpec):
        raise ValueError(f"spec must be an ActionSpec, not {type(spec).__name__}")
    if actions is not None and not isinstance(actions, runtime.DeviceMatrix) and not hasattr(actions, "__cuda_array_interface__"):
        actions = data._action_tensor(spec, actions)[0]  # (the uploaded matrix)
    tau = None
    for k in range(int(n_substeps)):
        tau = data.act(spec, actions, feed_forward=feed_forward, out=tau)
        data = step(model, data, joint_force_references=tau, inplace=inplace or k > 0)
    return data


def rollout(model: JaxSimModel, data: JaxSimModelData, n_steps: int, *, link_forces=None,
            joint_force_references=None, return_trajectory: bool = False):  # fmt: skip
    """``n_steps`` back-to-back steps (what ``jax.lax.fori_loop`` / ``jax.lax.scan`` over ``step`` does in the
    reference's notebooks); the input data is not modified.  ``joint_force_references``: constant over the steps
    (``[N, n]`` / ``[n]``), or -- [round 4] -- a SEQUENCE ``[n_steps, N, n]`` (``[n_steps, n]`` for one environment):
    step ``k`` applies ``joint_force_references[k]`` (``jxs_rollout_controlled``: one launch with the state in
    registers where the steps fuse).  ``return_trajectory=True`` [round 4]: returns ``(data, states)`` with
    ``states`` the host array ``[n_steps, rows, N]`` of the state block after every step (``jxs_rollout_recorded``: the
    stacked outputs of the reference's ``scan``; ``JaxSimModelData.from_state_block(model, states[k])`` rebuilds step k)."""
    dm = runtime.device_model(model, data.dtype)
    N, nL, n = data.batch_size, model.number_of_links(), model.dofs()
    if int(n_steps) <= 0:  # [ADVICE r4] nothing to do -- whatever shape the references have
        same = JaxSimModelData(model, data._state.copy(), data.velocity_representation, data._batched)
        return (same, np.zeros((0, data._state.rows, N), dtype=data.dtype)) if return_trajectory else same
    f = _as_device(link_forces, nL * 6, N, data.dtype, (nL, 6), data._state.tile)
    out = data._state.copy()
    seq = None
    if n == 0:
        joint_force_references = None  # (no joints: nothing to apply, whatever shape was handed over)
    if joint_force_references is not None and not isinstance(joint_force_references, DeviceArray) and \
            getattr(joint_force_references, "__cuda_array_interface__", None) is None:
        a = np.asarray(joint_force_references, dtype=np.float64)
        if a.ndim == 3 or (a.ndim == 2 and N == 1 and n > 0 and a.shape == (int(n_steps), n) and int(n_steps) != N):
            a = a.reshape(int(n_steps), N, n) if a.ndim == 2 else a
            if a.shape != (int(n_steps), N, n):
                raise ValueError((a.shape, (int(n_steps), N, n)))
            # rows k * n + j of the [n_steps * n][N] block: torque of joint j at step k
            seq = DeviceArray.from_host(np.ascontiguousarray(a.transpose(0, 2, 1).reshape(int(n_steps) * n, N)), tile=data._state.tile, dtype=data.dtype)
    if return_trajectory:
        K, rows = int(n_steps), data._state.shape[0]
        if K <= 0:
            return JaxSimModelData(model, out, data.velocity_representation, data._batched), np.zeros((0, rows, N), dtype=data.dtype)
        tau = seq if seq is not None else _as_device(joint_force_references, n, N, data.dtype, (n,), data._state.tile)
        traj = DeviceArray(K * rows, N, data.dtype, tile=data._state.tile)
        _lib.check(
            _lib.load().jxs_rollout_recorded(
                dm.handle, C.c_void_p(out.ptr), _ptr(tau), 1 if seq is not None else 0, _ptr(f),
                int(data.velocity_representation), N, K, C.c_void_p(traj.ptr), runtime._sp(),
            ),
            "jxs_rollout_recorded",
        )  # fmt: skip
        return JaxSimModelData(model, out, data.velocity_representation, data._batched), traj.to_host().reshape(K, rows, N)
    if seq is not None and n > 0 and int(n_steps) > 0:
        _lib.check(
            _lib.load().jxs_rollout_controlled(
                dm.handle, C.c_void_p(out.ptr), C.c_void_p(seq.ptr), _ptr(f), int(data.velocity_representation), N,
                int(n_steps), runtime._sp(),
            ),
            "jxs_rollout_controlled",
        )  # fmt: skip
        return JaxSimModelData(model, out, data.velocity_representation, data._batched)
    tau = _as_device(joint_force_references, n, N, data.dtype, (n,), data._state.tile)
    _lib.check(
        _lib.load().jxs_rollout(
            dm.handle, C.c_void_p(out.ptr), _ptr(tau), _ptr(f), int(data.velocity_representation), N,
            int(n_steps), runtime._sp(),
        ),
        "jxs_rollout",
    )  # fmt: skip
    return JaxSimModelData(model, out, data.velocity_representation, data._batched)


def _mixed_frame(data: JaxSimModelData):
    """(W_H_C, W_v_WC) of the active representation (``api/model.py:1356-1398``)."""
    N = data.batch_size
    H = data._base_transform_batched()
    rep = data.velocity_representation
    if rep == VelRepr.Inertial:
        return np.broadcast_to(np.eye(4), (N, 4, 4)), np.zeros((N, 6))
    if rep == VelRepr.Body:
        return H, data._base_velocity_batched(VelRepr.Inertial)
    Hm = H.copy()
    Hm[:, :3, :3] = np.eye(3)
    v = np.zeros((N, 6))
    v[:, :3] = data._base_velocity_batched(VelRepr.Mixed)[:, :3]
    return Hm, v


def _vx(v6: np.ndarray, x6: np.ndarray) -> np.ndarray:
    """``Cross.vx(v) @ x`` (``src/jaxsim/math/cross.py:14-43``), batched."""
    v, w = v6[:, :3], v6[:, 3:]
    return np.concatenate([np.cross(w, x6[:, :3]) + np.cross(v, x6[:, 3:]), np.cross(w, x6[:, 3:])], -1)


def _forward_dynamics_device(model: JaxSimModel, data: JaxSimModelData, entry: str, joint_forces, link_forces):
    """The shared body of ``forward_dynamics_aba`` / ``forward_dynamics_crb``: inputs to the device, one launch of the C
    entry point ``entry`` (both take the same arguments), the inertial-fixed base acceleration of the kernel moved to the
    active representation of ``data`` (``to_active``)."""
    dm = runtime.device_model(model, data.dtype)
    if entry == "jxs_forward_dynamics_crb":
        from .. import specialize

        specialize.ensure_mode(dm, model, specialize.MODE_FD_CRB)  # (first call: cached object, or built when hipcc is there)
    N, nL, n = data.batch_size, model.number_of_links(), model.dofs()
    f = _as_device(link_forces, nL * 6, N, data.dtype, (nL, 6), data._state.tile)
    tau = _as_device(joint_forces, n, N, data.dtype, (n,), data._state.tile)
    out = DeviceArray(6 + n, N, data.dtype, tile=data._state.tile)
    _lib.check(
        getattr(_lib.load(), entry)(
            dm.handle, C.c_void_p(data._state.ptr), _ptr(tau), _ptr(f), int(data.velocity_representation),
            C.c_void_p(out.ptr), N, runtime._sp(),
        ),
        entry,
    )  # fmt: skip
    res = out.to_host().T.astype(np.float64)
    W_vd, sdd = res[:, :6], res[:, 6:]
    if model.floating_base():
        W_H_C, W_v_WC = _mixed_frame(data)
        W_v_WB = data._base_velocity_batched(VelRepr.Inertial)
        C_vd = _inertial_to_other(W_vd - _vx(W_v_WC, W_v_WB), VelRepr.Body, W_H_C, False)
    else:
        C_vd = np.zeros((N, 6))
    return data._out(C_vd.astype(data.dtype)), data._out(sdd.astype(data.dtype))


def forward_dynamics_aba(model: JaxSimModel, data: JaxSimModelData, *, joint_forces=None, link_forces=None):
    """``forward_dynamics_aba`` (``src/jaxsim/api/model.py:1269-1406``): base acceleration in
    the active representation of ``data`` and joint accelerations."""
    return _forward_dynamics_device(model, data, "jxs_forward_dynamics_aba", joint_forces, link_forces)


def forward_dynamics_crb(model: JaxSimModel, data: JaxSimModelData, *, joint_forces=None, link_forces=None):
    """``forward_dynamics_crb`` (``src/jaxsim/api/model.py:1409-1498``): ``M nu_dot = B tau - h + J^T f`` solved in ONE
    launch (``jxs_forward_dynamics_crb``, ``MODE_FD_CRB``): the composite inertias of CRBA, one RNEA pass at zero
    acceleration with the link wrenches applied, the tree-sparse ``L^T D L`` factorisation of ``M``.  Same return
    convention as ``forward_dynamics_aba``.  Like the reference's CRB path the link wrenches act through the link
    Jacobians: for a model whose base link has a pose offset that differs from ``forward_dynamics_aba`` when
    ``link_forces`` are given in Body or Mixed representation.

    float32: ``M`` is ill-conditioned in joint coordinates on long serial chains (condition number 1e6 for 64 links), and
    a float32 factorisation of it -- this kernel's as much as ``numpy.linalg.solve`` on the reference's float32 ``M`` --
    loses up to 1e-2 of the largest acceleration there.  The float32 kernel therefore corrects its solution with one
    residual step (a second RNEA pass with the solution, the factor reused).  Measured worst error against the float64
    restatement over 323 random trees (host emulation of the kernel, ``profiles/query_modes_fuzz_campaign.txt``), floating
    serial chains by length: up to 48 links 6e-6, 49 .. 56 links 6.5e-5, 57 .. 64 links 3.0e-4 (the reference's
    formulation in float32 on the same states: 4e-4, 1.1e-3, 1.0e-2; without the residual step 1.6e-3, 4.7e-3, 1.3e-2).
    The articulated-body path measures about the same on such chains (2e-4 on 64 links) and is the faster kernel: for long
    serial chains in float32 ``forward_dynamics(..., prefer_aba=True)`` remains the one to use."""
    return _forward_dynamics_device(model, data, "jxs_forward_dynamics_crb", joint_forces, link_forces)


def forward_dynamics(model: JaxSimModel, data: JaxSimModelData, *, joint_forces=None, link_forces=None, prefer_aba: bool = True):
    """``forward_dynamics`` (``src/jaxsim/api/model.py:1231-1266``): ``forward_dynamics_aba``, or with
    ``prefer_aba=False`` ``forward_dynamics_crb``."""
    fn = forward_dynamics_aba if prefer_aba else forward_dynamics_crb
    return fn(model, data, joint_forces=joint_forces, link_forces=link_forces)


def total_mass(model: JaxSimModel) -> float:
    """``total_mass`` (``src/jaxsim/api/model.py:888``): the sum of the link masses."""
    return model.total_mass()


def inverse_dynamics(model: JaxSimModel, data: JaxSimModelData, *, joint_accelerations=None,
                     base_acceleration=None, link_forces=None):  # fmt: skip
    """``inverse_dynamics`` (``src/jaxsim/api/model.py:1746-1894``): base wrench in the active
    representation and joint torques."""
    dm = runtime.device_model(model, data.dtype)
    _check_quaternion(model, data, normalized=True)  # RNEA receives the raw quaternion (api/model.py:1856)
    N, nL, n = data.batch_size, model.number_of_links(), model.dofs()
    sdd = np.zeros((N, n)) if (joint_accelerations is None or n == 0) else np.broadcast_to(
        np.asarray(joint_accelerations, dtype=np.float64).reshape(-1, n), (N, n))  # fmt: skip  (n == 0: a model without joints takes the empty array the reference takes)
    vd = np.zeros((N, 6)) if base_acceleration is None else np.broadcast_to(
        np.asarray(base_acceleration, dtype=np.float64).reshape(-1, 6), (N, 6))  # fmt: skip
    # active representation -> inertial (api/model.py:1801-1842)
    W_H_C, W_v_WC = _mixed_frame(data)
    C_v_WC = _inertial_to_other(W_v_WC, VelRepr.Body, W_H_C, False)
    W_vd = _other_to_inertial(vd + _vx(C_v_WC, data._base_velocity_batched()), VelRepr.Body, W_H_C, False)
    in_acc = DeviceArray.from_host(
        np.ascontiguousarray(np.concatenate([W_vd, sdd], -1).T), tile=data._state.tile, dtype=data.dtype
    )
    f = _as_device(link_forces, nL * 6, N, data.dtype, (nL, 6), data._state.tile)
    out = DeviceArray(6 + n, N, data.dtype, tile=data._state.tile)
    _lib.check(
        _lib.load().jxs_inverse_dynamics(
            dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(in_acc.ptr), _ptr(f),
            int(data.velocity_representation), C.c_void_p(out.ptr), N, runtime._sp(),
        ),
        "jxs_inverse_dynamics",
    )  # fmt: skip
    res = out.to_host().T.astype(np.float64)
    f_B = _inertial_to_other(res[:, :6], data.velocity_representation, data._base_transform_batched(), True)
    return data._out(f_B.astype(data.dtype)), data._out(res[:, 6:].astype(data.dtype))


def free_floating_gravity_forces(model: JaxSimModel, data: JaxSimModelData):
    """``g(q)`` (``src/jaxsim/api/model.py:1897-1931``)."""
    z = data.replace(
        model,
        joint_velocities=np.zeros_like(data._fields()["joint_velocities"]),
        base_linear_velocity=np.zeros((data.batch_size, 3)),
        base_angular_velocity=np.zeros((data.batch_size, 3)),
    )
    fB, tau = inverse_dynamics(model, z)
    return np.concatenate([fB, tau], axis=-1)


def gravity_compensation_torques(model: JaxSimModel, data: JaxSimModelData, out: DeviceArray | None = None) -> DeviceArray:
    """Joint part of ``free_floating_gravity_forces`` as a device array ``[n][N]`` that ``step``
    accepts as ``joint_force_references`` without a host round trip (extension; the reference
    idiom is ``tau = js.model.free_floating_gravity_forces(model, data)[6:]`` followed by ``step``)."""
    dm = runtime.device_model(model, data.dtype)
    from .. import specialize

    specialize.ensure_mode(dm, model, specialize.MODE_GRAV)  # (first call: cached object, or built when hipcc is there)
    N, n = data.batch_size, model.dofs()
    out = out if out is not None else DeviceArray(n, N, data.dtype, tile=data._state.tile)
    _lib.check(
        _lib.load().jxs_gravity_torques(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), N, runtime._sp()),
        "jxs_gravity_torques",
    )
    return out


def _mixed_to_repr_block(data: JaxSimModelData) -> np.ndarray:
    """[N, 6, 6] matrices X with  v_mixed = X v_repr  for the base velocity in ``data.velocity_representation``
    (the inverse-transpose-free form of ``_transform_M_block``, ``src/jaxsim/api/model.py:1529-1551``)."""
    N = data.batch_size
    H = data._base_transform_batched()
    X = np.zeros((N, 6, 6))
    rep = data.velocity_representation
    if rep == VelRepr.Mixed:
        X[:] = np.eye(6)
    elif rep == VelRepr.Body:
        X[:, :3, :3] = H[:, :3, :3]
        X[:, 3:, 3:] = H[:, :3, :3]
    else:  # inertial-fixed: v_mixed,lin = v_lin + w x p_B
        p = H[:, :3, 3]
        X[:, :3, :3] = np.eye(3)
        X[:, 3:, 3:] = np.eye(3)
        X[:, 0, 4], X[:, 0, 5] = p[:, 2], -p[:, 1]
        X[:, 1, 3], X[:, 1, 5] = -p[:, 2], p[:, 0]
        X[:, 2, 3], X[:, 2, 4] = p[:, 1], -p[:, 0]
    return X


def free_floating_mass_matrix(model: JaxSimModel, data: JaxSimModelData):
    """``M(q)`` in the active velocity representation (``src/jaxsim/api/model.py:1553-1590``): ONE launch of
    the composite-rigid-body kernel (``jxs_mass_matrix``, ``rbda/crba.py:10-170``), which returns the matrix
    in Mixed representation; Body / Inertial are the block congruence ``diag(X, I)^T M diag(X, I)``."""
    dm = runtime.device_model(model, data.dtype)
    N, n = data.batch_size, model.dofs()
    nv = 6 + n
    out = DeviceArray(nv * nv, N, data.dtype, tile=data._state.tile)
    _lib.check(
        _lib.load().jxs_mass_matrix(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), N, runtime._sp()),
        "jxs_mass_matrix",
    )
    M = out.to_host().T.astype(np.float64).reshape(N, nv, nv)
    if data.velocity_representation != VelRepr.Mixed:
        X = _mixed_to_repr_block(data)
        Xt = np.transpose(X, (0, 2, 1))
        M = M.copy()
        Mbb, Mbj = M[:, :6, :6].copy(), M[:, :6, 6:].copy()
        M[:, :6, :6] = Xt @ Mbb @ X
        M[:, :6, 6:] = Xt @ Mbj
        M[:, 6:, :6] = np.transpose(M[:, :6, 6:], (0, 2, 1))
    return data._out(M.astype(data.dtype))


def free_floating_mass_matrix_inverse(model: JaxSimModel, data: JaxSimModelData):
    """``M(q)^-1`` in the active velocity representation (``src/jaxsim/api/model.py:1593-1631``; the reference
    runs its ``mass_inverse`` recursion, ``rbda/mass_inverse.py:11-233``): ONE launch of ``jxs_mass_matrix_inverse``
    (columns = responses of the articulated-body factorisation to unit generalized forces, Mixed
    representation), then the block congruence ``diag(X^-1, I) M^-1 diag(X^-1, I)^T`` for Body / Inertial."""
    dm = runtime.device_model(model, data.dtype)
    N, n = data.batch_size, model.dofs()
    nv = 6 + n
    out = DeviceArray(nv * nv, N, data.dtype, tile=data._state.tile)
    _lib.check(
        _lib.load().jxs_mass_matrix_inverse(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), N, runtime._sp()),
        "jxs_mass_matrix_inverse",
    )
    Mi = out.to_host().T.astype(np.float64).reshape(N, nv, nv)
    Mi = 0.5 * (Mi + np.transpose(Mi, (0, 2, 1)))
    if data.velocity_representation != VelRepr.Mixed:
        Xi = np.linalg.inv(_mixed_to_repr_block(data))
        Xit = np.transpose(Xi, (0, 2, 1))
        Mbb, Mbj = Mi[:, :6, :6].copy(), Mi[:, :6, 6:].copy()
        Mi[:, :6, :6] = Xi @ Mbb @ Xit
        Mi[:, :6, 6:] = Xi @ Mbj
        Mi[:, 6:, :6] = np.transpose(Mi[:, :6, 6:], (0, 2, 1))
    return data._out(Mi.astype(data.dtype))


def _adjoint(H: np.ndarray, inverse: bool = False) -> np.ndarray:
    """Batched ``Adjoint.from_transform`` (``src/jaxsim/math/adjoint.py:46-107``): ``[[R, S(p) R], [0, R]]``."""
    R, p = H[..., :3, :3], H[..., :3, 3]
    if inverse:  # (R, p)^-1 = (R^T, -R^T p)
        R = np.swapaxes(R, -1, -2)
        p = -np.einsum("...ij,...j->...i", R, p)
    Sp = np.zeros(R.shape)
    Sp[..., 0, 1], Sp[..., 0, 2] = -p[..., 2], p[..., 1]
    Sp[..., 1, 0], Sp[..., 1, 2] = p[..., 2], -p[..., 0]
    Sp[..., 2, 0], Sp[..., 2, 1] = -p[..., 1], p[..., 0]
    X = np.zeros(R.shape[:-2] + (6, 6))
    X[..., :3, :3] = R
    X[..., :3, 3:] = Sp @ R
    X[..., 3:, 3:] = R
    return X


def _vx_matrix(v6: np.ndarray) -> np.ndarray:
    """Batched ``Cross.vx`` (``src/jaxsim/math/cross.py:14-43``): ``[[S(w), S(v)], [0, S(w)]]``."""
    def S(a):
        out = np.zeros(a.shape[:-1] + (3, 3))
        out[..., 0, 1], out[..., 0, 2] = -a[..., 2], a[..., 1]
        out[..., 1, 0], out[..., 1, 2] = a[..., 2], -a[..., 0]
        out[..., 2, 0], out[..., 2, 1] = -a[..., 1], a[..., 0]
        return out

    X = np.zeros(v6.shape[:-1] + (6, 6))
    X[..., :3, :3] = S(v6[..., 3:])
    X[..., :3, 3:] = S(v6[..., :3])
    X[..., 3:, 3:] = S(v6[..., 3:])
    return X


def _support_mask(model: JaxSimModel) -> np.ndarray:
    """``hstack([ones(5), kappa_bool])`` per link (``src/jaxsim/api/model.py:975-981``): ``[nL, 6+n]``."""
    kdp = model.kin_dyn_parameters
    nL = kdp.number_of_links()
    mask = np.zeros((nL, 6 + nL - 1))
    mask[:, :6] = 1.0
    for L in range(nL):
        j = L
        while j > 0:
            mask[L, 6 + j - 1] = 1.0
            j = int(kdp.parent_array[j])
    return mask


def jacobian_full_doubly_left(model: JaxSimModel, data: JaxSimModelData):
    """``jaxsim.rbda.jacobian_full_doubly_left`` + ``jacobian_derivative_full_doubly_left``
    (``src/jaxsim/rbda/jacobian.py:128-339``) in ONE launch of the Jacobian kernel (``jxs_jacobian_full``):
    ``(B_J_full [N,6,6+n], B_Jdot_full [N,6,6+n], B_H_L [N,nL,4,4])`` as float64 host arrays."""
    dm = runtime.device_model(model, data.dtype)
    N, n, nL = data.batch_size, model.dofs(), model.number_of_links()
    nv = 6 + n
    out = DeviceArray(12 * nv, N, data.dtype, tile=data._state.tile)
    outH = DeviceArray(12 * nL, N, data.dtype, tile=data._state.tile)
    _lib.check(
        _lib.load().jxs_jacobian_full(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), C.c_void_p(outH.ptr), N, runtime._sp()),
        "jxs_jacobian_full",
    )
    JJ = out.to_host().T.astype(np.float64)
    H = np.zeros((N, nL, 4, 4))
    H[:, :, :3, :] = outH.to_host().T.astype(np.float64).reshape(N, nL, 3, 4)
    H[:, :, 3, 3] = 1.0
    return JJ[:, : 6 * nv].reshape(N, 6, nv), JJ[:, 6 * nv :].reshape(N, 6, nv), H


def _block_T(X: np.ndarray, n: int, identity: bool = True) -> np.ndarray:
    T = np.zeros(X.shape[:-2] + (6 + n, 6 + n))
    T[..., :6, :6] = X
    if identity:
        T[..., 6:, 6:] = np.eye(n)
    return T


def generalized_free_floating_jacobian(model: JaxSimModel, data: JaxSimModelData, *, output_vel_repr=None):
    """Free-floating Jacobians of all links, ``[nL, 6, 6+n]`` (``src/jaxsim/api/model.py:925-1045``): the
    generalized velocity is expressed in ``data.velocity_representation``, the link velocity in
    ``output_vel_repr`` (default: the same).  One launch of the Jacobian kernel; the column masks and the
    6x6 input / output transforms are applied on the host like the reference applies them after its
    ``rbda`` call."""
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    N, n = data.batch_size, model.dofs()
    B_J_full, _, B_H_L = jacobian_full_doubly_left(model, data)
    W_H_B = data._base_transform_batched()
    rep = data.velocity_representation
    if rep == VelRepr.Inertial:
        B_X_I = _adjoint(W_H_B, inverse=True)
    elif rep == VelRepr.Body:
        B_X_I = np.broadcast_to(np.eye(6), (N, 6, 6))
    else:
        BW_H_B = W_H_B.copy()
        BW_H_B[:, :3, 3] = 0.0
        B_X_I = _adjoint(BW_H_B, inverse=True)
    B_J_full_I = B_J_full @ _block_T(B_X_I, n)
    B_J_WL_I = _support_mask(model)[None, :, None, :] * B_J_full_I[:, None]  # [N, nL, 6, nv]
    if out_rep == VelRepr.Inertial:
        O_X_B = _adjoint(W_H_B)[:, None]
    elif out_rep == VelRepr.Body:
        O_X_B = _adjoint(B_H_L, inverse=True)
    else:
        LW_H_L = W_H_B[:, None] @ B_H_L
        LW_H_L[..., :3, 3] = 0.0
        O_X_B = _adjoint(LW_H_L @ np.linalg.inv(B_H_L))
    return data._out((O_X_B @ B_J_WL_I).astype(data.dtype))


def generalized_free_floating_jacobian_derivative(model: JaxSimModel, data: JaxSimModelData, *, output_vel_repr=None):
    """Time derivative of the free-floating Jacobians of all links, ``[nL, 6, 6+n]``
    (``src/jaxsim/api/model.py:1046-1228``): ``O_Jdot = O_Xdot_B B_J T + O_X_B B_Jdot T + O_X_B B_J Tdot`` with the
    doubly-left Jacobian and its derivative from one launch of the Jacobian kernel."""
    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    N, n, nL = data.batch_size, model.dofs(), model.number_of_links()
    B_J_full, B_Jd_full, B_H_L = jacobian_full_doubly_left(model, data)
    mask = _support_mask(model)[None, :, None, :]
    B_Jd_WL_B = mask * B_Jd_full[:, None]
    B_J_WL_B = mask * B_J_full[:, None]
    W_H_B = data._base_transform_batched()
    rep = data.velocity_representation
    B_v_WB = np.asarray(data._base_velocity_batched(VelRepr.Body), np.float64)
    # ---- input representation: T and its derivative (:1104-1146)
    if rep == VelRepr.Inertial:
        B_X_W = _adjoint(W_H_B, inverse=True)
        W_v_WB = np.asarray(data._base_velocity_batched(VelRepr.Inertial), np.float64)
        X, Xd = B_X_W, -B_X_W @ _vx_matrix(W_v_WB)
    elif rep == VelRepr.Body:
        X, Xd = np.broadcast_to(np.eye(6), (N, 6, 6)), np.zeros((N, 6, 6))
    else:
        BW_H_B = W_H_B.copy()
        BW_H_B[:, :3, 3] = 0.0
        B_X_BW = _adjoint(BW_H_B, inverse=True)
        BW_v_WB = np.asarray(data._base_velocity_batched(VelRepr.Mixed), np.float64)
        BW_v_BW_B = BW_v_WB.copy()
        BW_v_BW_B[:, :3] = 0.0  # BW_v_WB - BW_v_W_BW, the latter being the linear part
        X, Xd = B_X_BW, -B_X_BW @ _vx_matrix(BW_v_BW_B)
    T, Td = _block_T(X, n)[:, None], _block_T(Xd, n, identity=False)[:, None]
    # ---- output representation: O_X_B and its derivative (:1148-1214)
    if out_rep == VelRepr.Inertial:
        W_X_B = _adjoint(W_H_B)
        O_X_B, O_Xd_B = W_X_B[:, None], (W_X_B @ _vx_matrix(B_v_WB))[:, None]
    elif out_rep == VelRepr.Body:
        L_X_B = _adjoint(B_H_L, inverse=True)
        B_X_L = _adjoint(B_H_L)
        nu_B = np.concatenate([B_v_WB, np.asarray(data._fields()["joint_velocities"], np.float64).reshape(N, n)], -1)
        L_v_WL = np.einsum("nlij,nj->nli", L_X_B @ B_J_WL_B, nu_B)
        O_X_B = L_X_B
        O_Xd_B = -L_X_B @ _vx_matrix(np.einsum("nlij,nlj->nli", B_X_L, L_v_WL) - B_v_WB[:, None])
    else:
        W_H_L = W_H_B[:, None] @ B_H_L
        LW_H_L = W_H_L.copy()
        LW_H_L[..., :3, 3] = 0.0
        LW_H_B = LW_H_L @ np.linalg.inv(B_H_L)
        LW_X_B = _adjoint(LW_H_B)
        B_X_LW = _adjoint(LW_H_B, inverse=True)
        nu_B = np.concatenate([B_v_WB, np.asarray(data._fields()["joint_velocities"], np.float64).reshape(N, n)], -1)
        LW_v_WL = np.einsum("nlij,nj->nli", LW_X_B @ B_J_WL_B, nu_B)
        LW_v_W_LW = LW_v_WL.copy()
        LW_v_W_LW[..., 3:] = 0.0
        LW_v_LW_L = LW_v_WL - LW_v_W_LW
        LW_v_B_LW = LW_v_WL - np.einsum("nlij,nj->nli", LW_X_B, B_v_WB) - LW_v_LW_L
        O_X_B = LW_X_B
        O_Xd_B = -LW_X_B @ _vx_matrix(np.einsum("nlij,nlj->nli", B_X_LW, LW_v_B_LW))
    Jd = O_Xd_B @ B_J_WL_B @ T + O_X_B @ B_Jd_WL_B @ T + O_X_B @ B_J_WL_B @ Td
    return data._out(Jd.astype(data.dtype))


def free_floating_bias_forces(model: JaxSimModel, data: JaxSimModelData):
    """``h(q, nu)`` (``src/jaxsim/api/model.py:1934-1978``); fixed-base models drop the base
    velocity like the reference does."""
    d = data
    if not model.floating_base():
        d = data.replace(
            model,
            base_linear_velocity=np.zeros((data.batch_size, 3)),
            base_angular_velocity=np.zeros((data.batch_size, 3)),
        )
    fB, tau = inverse_dynamics(model, d)
    return np.concatenate([fB, tau], axis=-1)


# ---- momentum and energy (src/jaxsim/api/model.py:888-925, 1988-2175, 2397-2453): one launch of the centroidal
#      kernel (js.com, jxs_centroidal), cached on the data object, and the reference's 6x6 transforms on the host


def link_spatial_inertia_matrices(model: JaxSimModel) -> np.ndarray:
    """``link_spatial_inertia_matrices`` (``src/jaxsim/api/model.py:900-917``): [nL, 6, 6] in the link frames,
    ``[[m 1, m S(c)^T], [m S(c), I_c + m S(c) S(c)^T]]`` (``math/inertia.py:14-41``), from the model tables."""
    from .com import _skew

    kdp = model.kin_dyn_parameters
    m = np.asarray(kdp.link_mass, np.float64)[:, None, None]
    S = _skew(np.asarray(kdp.link_com, np.float64))
    M = np.zeros((m.shape[0], 6, 6))
    M[:, :3, :3] = m * np.eye(3)
    M[:, :3, 3:] = m * np.swapaxes(S, -1, -2)
    M[:, 3:, :3] = m * S
    M[:, 3:, 3:] = np.asarray(kdp.link_inertia_com, np.float64) + m * (S @ np.swapaxes(S, -1, -2))
    return M


def _repr_block(data: JaxSimModelData, rep) -> np.ndarray:
    """``_mixed_to_repr_block`` for the representation ``rep``."""
    with data.switch_velocity_representation(rep):
        return _mixed_to_repr_block(data)


def _force_shift(d: np.ndarray) -> np.ndarray:
    """[N, 6, 6] force transform that moves the reference point of a wrench by -d (world axes): [f; n + d x f]."""
    from .com import _skew

    X = np.zeros(d.shape[:-1] + (6, 6))
    X[..., :3, :3] = np.eye(3)
    X[..., 3:, 3:] = np.eye(3)
    X[..., 3:, :3] = _skew(d)
    return X


def total_momentum_jacobian(model: JaxSimModel, data: JaxSimModelData, *, output_vel_repr=None):
    """``total_momentum_jacobian`` (``src/jaxsim/api/model.py:2024-2087``): ``free_floating_mass_matrix[0:6]`` with
    the output in ``output_vel_repr`` (default: the data's), [6, 6+n] / [N, 6, 6+n].  From the centroidal momentum
    matrix: moved from the CoM to the base position, then the 6x6 congruences of the mass matrix."""
    from .com import COM, _centroidal

    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    rec, A_G = _centroidal(model, data, jacobian=True)
    c = rec[:, COM : COM + 3] - data._base_transform_batched()[:, :3, 3]
    Jh = _force_shift(c) @ A_G  # about the base position, world axes: frame C = the Mixed representation
    Jh[:, :, :6] = Jh[:, :, :6] @ _mixed_to_repr_block(data)
    Jh = np.swapaxes(_repr_block(data, out_rep), -1, -2) @ Jh
    return data._out(Jh.astype(data.dtype))


def locked_spatial_inertia(model: JaxSimModel, data: JaxSimModelData):
    """``locked_spatial_inertia`` (``src/jaxsim/api/model.py:1993-2007``): ``total_momentum_jacobian[:, 0:6]``, from
    the record alone (the locked centroidal inertia moved to the base position)."""
    from .com import COM, _centroidal, _locked_G_world

    rec, _ = _centroidal(model, data)
    F = _force_shift(rec[:, COM : COM + 3] - data._base_transform_batched()[:, :3, 3])
    X = _mixed_to_repr_block(data)
    M = np.swapaxes(X, -1, -2) @ F @ _locked_G_world(model, data) @ np.swapaxes(F, -1, -2) @ X
    return data._out(M.astype(data.dtype))


def total_momentum(model: JaxSimModel, data: JaxSimModelData):
    """``total_momentum`` (``src/jaxsim/api/model.py:2010-2021``): ``total_momentum_jacobian @ nu`` in the data's
    representation, from the record (the centroidal momentum moved to the world origin, then to the data's frame)."""
    from .com import COM, MOMENTUM, _centroidal

    rec, _ = _centroidal(model, data)
    h = rec[:, MOMENTUM : MOMENTUM + 6].copy()
    h[:, 3:] += np.cross(rec[:, COM : COM + 3], h[:, :3])
    h = _inertial_to_other(h, data.velocity_representation, data._base_transform_batched(), True)
    return data._out(h.astype(data.dtype))


def _avg_velocity_transform(model: JaxSimModel, data: JaxSimModelData, out_rep) -> np.ndarray:
    """The motion transforms of ``average_velocity_jacobian`` (``src/jaxsim/api/model.py:2127-2157``): W_X_GW, B_X_GB or
    BW_X_GW (translations), applied -- like the reference -- to the average centroidal velocity of the data's G frame."""
    from .com import COM, _centroidal, _skew

    rec, _ = _centroidal(model, data)
    H = data._base_transform_batched()
    p = rec[:, COM : COM + 3]
    if out_rep == VelRepr.Body:
        p = np.einsum("nji,nj->ni", H[:, :3, :3], p - H[:, :3, 3])
    elif out_rep == VelRepr.Mixed:
        p = p - H[:, :3, 3]
    X = np.zeros(p.shape[:-1] + (6, 6))
    X[:, :3, :3] = np.eye(3)
    X[:, 3:, 3:] = np.eye(3)
    X[:, :3, 3:] = _skew(p)
    return X


def average_velocity_jacobian(model: JaxSimModel, data: JaxSimModelData, *, output_vel_repr=None):
    """``average_velocity_jacobian`` (``src/jaxsim/api/model.py:2108-2157``), [6, 6+n] / [N, 6, 6+n]."""
    from . import com

    out_rep = data.velocity_representation if output_vel_repr is None else VelRepr(output_vel_repr)
    G_J = com.average_centroidal_velocity_jacobian(model, data)
    G_J = np.asarray(G_J, np.float64).reshape(data.batch_size, 6, 6 + model.dofs())
    return data._out((_avg_velocity_transform(model, data, out_rep) @ G_J).astype(data.dtype))


def average_velocity(model: JaxSimModel, data: JaxSimModelData):
    """``average_velocity`` (``src/jaxsim/api/model.py:2090-2105``): ``average_velocity_jacobian @ nu``, from the record."""
    from . import com

    v = np.asarray(com.average_centroidal_velocity(model, data), np.float64).reshape(data.batch_size, 6)
    X = _avg_velocity_transform(model, data, data.velocity_representation)
    return data._out(np.einsum("nij,nj->ni", X, v).astype(data.dtype))


def kinetic_energy(model: JaxSimModel, data: JaxSimModelData):
    """``kinetic_energy`` (``src/jaxsim/api/model.py:2415-2433``): 1/2 nu^T M nu (any representation)."""
    from .com import KINETIC, _centroidal

    rec, _ = _centroidal(model, data)
    return data._out(rec[:, KINETIC].astype(data.dtype))


def potential_energy(model: JaxSimModel, data: JaxSimModelData):
    """``potential_energy`` (``src/jaxsim/api/model.py:2436-2453``) AS THE REFERENCE COMPUTES IT: ``m z_CoM gravity``
    with ``model.gravity = -9.81``, i.e. ``-m g z`` -- NEGATIVE for a CoM above the ground.  So the physical potential
    energy is ``-potential_energy`` and ``kinetic_energy - potential_energy`` is what a conservative motion keeps."""
    from .com import POTENTIAL, _centroidal

    rec, _ = _centroidal(model, data)
    return data._out(rec[:, POTENTIAL].astype(data.dtype))


def mechanical_energy(model: JaxSimModel, data: JaxSimModelData):
    """``mechanical_energy`` (``src/jaxsim/api/model.py:2397-2412``): ``kinetic_energy + potential_energy`` like the
    reference -- which, with the sign of its ``potential_energy``, is NOT conserved (``K - U`` is)."""
    from .com import KINETIC, POTENTIAL, _centroidal

    rec, _ = _centroidal(model, data)
    return data._out((rec[:, KINETIC] + rec[:, POTENTIAL]).astype(data.dtype))


def link_bias_accelerations(model: JaxSimModel, data: JaxSimModelData) -> np.ndarray:
    """``link_bias_accelerations`` (``src/jaxsim/api/model.py:2179-2395``): ``J̇ν`` of every link in the data's velocity
    representation, [nL, 6] / [N, nL, 6] -- one launch of the frame kernel over all links (``api/frame.py``), shared with
    ``js.link.transform`` / ``velocity`` / ``bias_acceleration`` of the same state."""
    from . import frame as _frame

    rec, _ = _frame._record(model, data, _frame._ALL_LINKS, data.velocity_representation)
    return data._out(rec[:, :, _frame.BIAS : _frame.BIAS + 6].astype(data.dtype))


def forward_kinematics(model: JaxSimModel, data: JaxSimModelData) -> np.ndarray:
    """``forward_kinematics`` (``src/jaxsim/api/model.py:474-493``): ``W_H_L`` of all links, [nL, 4, 4] / [N, nL, 4, 4],
    from the cached kinematics (the kinematics kernel, ``MODE_KIN``)."""
    return data._link_transforms


# ---- Coriolis matrix (src/jaxsim/api/model.py:1634-1745): one launch of the Coriolis kernel (jxs_coriolis,
#      MODE_CORIOLIS), which returns C and M in Mixed representation; the other representations on the host


def coriolis_matrix_device(model: JaxSimModel, data: JaxSimModelData, *, out: DeviceArray | None = None,
                           out_mass_matrix: DeviceArray | None = None, mass_matrix: bool = False):  # fmt: skip
    """Extension for device-resident loops (like ``js.com.centroidal_quantities``): the free-floating Coriolis matrix in
    MIXED representation as a ``DeviceArray`` ``[(6+n)^2][N]`` (row-major, the layout of ``jxs_mass_matrix``) -- and with
    ``mass_matrix=True`` or ``out_mass_matrix`` the pair ``(C, M)``, the Mixed mass matrix of the same launch.  One
    launch, no host round trip; ``out`` / ``out_mass_matrix`` are reused when given."""
    from .. import specialize

    dm = runtime.device_model(model, data.dtype)
    specialize.ensure_mode(dm, model, specialize.MODE_CORIOLIS)  # (first call: cached object, or built when hipcc is there)
    N, nv = data.batch_size, 6 + model.dofs()
    tile = data._state.tile
    want = (nv * nv, N, np.dtype(data.dtype), tile)

    def buffer(b):
        b = b if b is not None else DeviceArray(nv * nv, N, data.dtype, tile=tile)
        if (b.rows, b.cols, b.dtype, b.tile) != want:
            raise ValueError(((b.rows, b.cols, b.dtype, b.tile), want))
        return b

    out = buffer(out)
    with_M = mass_matrix or out_mass_matrix is not None
    out_mass_matrix = buffer(out_mass_matrix) if with_M else None
    _lib.check(
        _lib.load().jxs_coriolis(dm.handle, C.c_void_p(data._state.ptr), C.c_void_p(out.ptr), _ptr(out_mass_matrix), N,
                                 runtime._sp()),
        "jxs_coriolis",
    )  # fmt: skip
    return (out, out_mass_matrix) if with_M else out


def _coriolis_mixed_to(rep, W_H_B: np.ndarray, BW_v_WB: np.ndarray, C_mixed: np.ndarray, M_mixed: np.ndarray) -> np.ndarray:
    """``C`` in representation ``rep`` from the Mixed ``C`` and ``M`` of the kernel: ``T^T (M Tdot + C T)`` with
    ``T = diag(X, 1)``, ``X`` = ``_mixed_to_repr_block`` (``v_mixed = X v_rep``) and its time derivative for the base
    velocity ``BW_v_WB`` (Mixed, [N, 6]): Body ``Xdot = diag(S(w) R, S(w) R)``, Inertial ``Xdot[0:3, 3:6] = -S(pdot)``."""
    from .com import _skew

    if rep == VelRepr.Mixed:
        return C_mixed
    N = C_mixed.shape[0]
    X, Xd = np.zeros((N, 6, 6)), np.zeros((N, 6, 6))
    if rep == VelRepr.Body:
        R = W_H_B[:, :3, :3]
        Rd = _skew(BW_v_WB[:, 3:]) @ R
        X[:, :3, :3] = X[:, 3:, 3:] = R
        Xd[:, :3, :3] = Xd[:, 3:, 3:] = Rd
    else:
        X[:, :3, :3] = X[:, 3:, 3:] = np.eye(3)
        X[:, :3, 3:] = -_skew(W_H_B[:, :3, 3])
        Xd[:, :3, 3:] = -_skew(BW_v_WB[:, :3])
    # T^T (M Tdot + C T): Tdot touches only columns 0:6, T only the base rows / columns
    out = C_mixed.copy()
    out[:, :, :6] = C_mixed[:, :, :6] @ X + M_mixed[:, :, :6] @ Xd
    out[:, :6, :] = np.transpose(X, (0, 2, 1)) @ out[:, :6, :]
    return out


def free_floating_coriolis_matrix(model: JaxSimModel, data: JaxSimModelData):
    """``free_floating_coriolis_matrix`` (``src/jaxsim/api/model.py:1634-1745``): ``C(q, nu)`` in the data's velocity
    representation, [6+n, 6+n] / [N, 6+n, 6+n].  ONE launch of the Coriolis kernel (``jxs_coriolis``) returns C and M in
    Mixed representation (a tree recursion over the composite inertia, not the reference's sum over dense link
    Jacobians); Body / Inertial are ``T^T (M Tdot + C T)`` on the host, as in the reference.  Like the reference, a
    fixed-base model keeps the stored base velocity in nu and the base block of C."""
    N, nv = data.batch_size, 6 + model.dofs()
    rep = data.velocity_representation
    if rep == VelRepr.Mixed:
        Cd = coriolis_matrix_device(model, data)
        Cm = Cd.to_host().T.astype(np.float64).reshape(N, nv, nv)
        return data._out(Cm.astype(data.dtype))
    Cd, Md = coriolis_matrix_device(model, data, mass_matrix=True)
    Cm = Cd.to_host().T.astype(np.float64).reshape(N, nv, nv)
    Mm = Md.to_host().T.astype(np.float64).reshape(N, nv, nv)
    v = np.asarray(data._base_velocity_batched(VelRepr.Mixed), np.float64)
    out = _coriolis_mixed_to(rep, data._base_transform_batched(), v, Cm, Mm)
    return data._out(out.astype(data.dtype))
