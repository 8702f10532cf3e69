"""What ``JaxSimModelData.observe``, ``.act``, ``.evaluate`` and ``.contact_sensors`` are told to do: ``ObservationSpec``,
``ActionSpec``, ``RewardSpec`` and ``ContactSensorSpec``, the term grammar they share and the constants of their tables
(``include/jaxsim_amd.h``).  A spec knows nothing of the object that holds a state block: ``jaxsim_amd.data`` imports this
module, never the other way round, and re-exports its public names."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, runtime
from .model import VelRepr
from .state import StateLayout

# kinds of an observation slot (JXS_OBS_* of include/jaxsim_amd.h)
OBS_STATE_ROW, OBS_SOURCE_ROW, OBS_BASE_QUAT_UNIT, OBS_BASE_ROTATION, OBS_BASE_VELOCITY, OBS_PROJECTED_GRAVITY = range(6)
OBS_MAX_WIDTH, OBS_MAX_SOURCES = 4096, 4


class _SpecTable:
    """The device table of a spec (``jxs_observation``, ``jxs_action``, ``jxs_evaluation``, ``jxs_contact_sensors`` of the four
    spec classes below): one per spec, uploaded at the first use -- one small allocation and a blocking copy -- and freed with
    the spec.  The table holds nothing of the model; the library checks it against the layout and dtype of the model of every
    launch, so one table serves every device model of the spec's layout.  A spec gives ``_create(dm, handle)``, which fills
    ``handle`` through the library's create call or raises, and names the library's destroy call in ``_destroy``."""

    _handle = None

    def _table(self, dm) -> C.c_void_p:
        if self._handle is None:
            h = C.c_void_p()
            self._create(dm, h)
            self._handle = h
        return self._handle

    def __del__(self):
        h, self._handle = self._handle, None
        if h is not None:
            try:
                getattr(_lib.load(), self._destroy)(h)
            except Exception:
                pass


def _term_slots(model, lay: StateLayout, term, name: str, opts: dict, src_names: list, src_rows: list, what: str):
    """``(slots, default key)`` of one named term of an ``ObservationSpec`` or a ``RewardSpec``: the ``(kind, source, index)``
    triples it stands for.  The options it understands are taken out of ``opts`` (``joints``; ``name``, ``rows``, ``take``);
    a source new to ``src_names`` / ``src_rows`` is appended to them.  ``ValueError`` for an unknown name, joint or row."""
    n = lay.n_joints
    state = lambda first, count: [(OBS_STATE_ROW, 0, first + k) for k in range(count)]  # noqa: E731
    kind = lambda k, comps: [(k, 0, c) for c in comps]  # noqa: E731
    fixed = {
        "base_position": state(lay.row_pos, 3),
        "base_height": state(lay.row_pos + 2, 1),
        "base_quaternion": state(lay.row_quat, 4),
        "base_orientation": kind(OBS_BASE_QUAT_UNIT, range(4)),
        "base_rotation": kind(OBS_BASE_ROTATION, range(9)),
        "base_velocity": kind(OBS_BASE_VELOCITY, range(6)),
        "base_linear_velocity": kind(OBS_BASE_VELOCITY, range(3)),
        "base_angular_velocity": kind(OBS_BASE_VELOCITY, range(3, 6)),
        "projected_gravity": kind(OBS_PROJECTED_GRAVITY, range(3)),
        "tangential_deformation": state(lay.row_m, 3 * lay.n_points),
    }
    if name in ("joint_positions", "joint_velocities"):
        first = lay.row_s if name == "joint_positions" else lay.row_sd
        joints = opts.pop("joints", None)
        if joints is None:
            idx = list(range(n))
        else:
            known = {nm: i for i, nm in enumerate(model.joint_names())}
            missing = [j for j in joints if j not in known]
            if missing:
                raise ValueError(f"term {name!r}: unknown joints {missing}")
            idx = [known[j] for j in joints]
        return [(OBS_STATE_ROW, 0, first + i) for i in idx], name
    if name == "source":
        sname, rows = opts.pop("name", None), opts.pop("rows", None)
        if not isinstance(sname, str) or not isinstance(rows, (int, np.integer)) or rows <= 0:
            raise ValueError(f"term {term!r}: a source needs name=<str> and rows=<positive int>")
        take = opts.pop("take", None)
        take = list(range(int(rows))) if take is None else [int(r) for r in take]
        if any(r < 0 or r >= rows for r in take):
            raise ValueError(f"source {sname!r}: rows {take} outside [0, {rows})")
        if sname in src_names:
            if src_rows[src_names.index(sname)] != int(rows):
                raise ValueError(f"source {sname!r} named with {rows} and with {src_rows[src_names.index(sname)]} rows")
        else:
            if len(src_names) == OBS_MAX_SOURCES:
                raise ValueError(f"more than {OBS_MAX_SOURCES} sources")
            src_names.append(sname)
            src_rows.append(int(rows))
        return [(OBS_SOURCE_ROW, src_names.index(sname), r) for r in take], sname
    if name in fixed:
        return fixed[name], name
    raise ValueError(f"unknown {what} term {name!r}")


def _per_element(name: str, what: str, value, count: int, dt) -> np.ndarray:
    """The option ``what`` of the term ``name`` as ``count`` float64 values (a scalar is repeated), each finite in ``dt``."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != count):
        raise ValueError(f"term {name!r}: {what} of shape {a.shape}: expected a scalar or {count} values")
    a = np.broadcast_to(a, (count,))
    with np.errstate(over="ignore"):
        if not (np.isfinite(a).all() and np.isfinite(a.astype(dt)).all()):
            raise ValueError(f"term {name!r}: {what} is not finite in {dt.name}")
    return a


class ObservationSpec(_SpecTable):
    """What ``JaxSimModelData.observe`` assembles for one model: an ordered list of terms, flattened into ``size`` slots
    ``(kind, source, index)`` with an offset and a scale each (the table of ``jxs_observation_create``).  Built once on the
    host -- no device is needed --, uploaded at the first ``observe``, used for every step of a loop.

    ``slots`` ``[size, 3]`` int32, ``offset`` / ``scale`` ``[size]`` float64, ``slices``: term key -> column slice,
    ``source_names`` / ``source_rows``: the auxiliary blocks ``observe`` must be given, in source order."""

    def __init__(self, layout: StateLayout, dtype, out_dtype, velocity_representation, slots, offset, scale, slices, source_names, source_rows):
        self.layout = layout
        self.dtype = np.dtype(dtype)
        self.out_dtype = np.dtype(out_dtype)
        self.velocity_representation = None if velocity_representation is None else VelRepr(velocity_representation)
        self.slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1, 3)
        self.offset = np.ascontiguousarray(offset, dtype=np.float64)
        self.scale = np.ascontiguousarray(scale, dtype=np.float64)
        self.slices = dict(slices)
        self.source_names, self.source_rows = tuple(source_names), tuple(int(r) for r in source_rows)

    @property
    def size(self) -> int:
        return self.slots.shape[0]

    @staticmethod
    def build(model, terms, *, dtype=np.float32, velocity_representation=None, out_dtype=None) -> "ObservationSpec":
        """``terms``: an ordered sequence of names or ``(name, options)``:

        * ``"joint_positions"``, ``"joint_velocities"`` -- option ``joints=[names]`` picks and orders a subset;
        * ``"base_position"``, ``"base_height"``, ``"base_quaternion"`` (as stored), ``"base_orientation"`` (unit norm, the
          rule of ``data.base_orientation``), ``"base_rotation"`` (row-major);
        * ``"base_velocity"``, ``"base_linear_velocity"``, ``"base_angular_velocity"`` (in ``velocity_representation``; ``None``
          = the data object's at the call), ``"projected_gravity"`` (``R^T (0, 0, -1)``), ``"tangential_deformation"``;
        * ``("source", dict(name=..., rows=...))``: an auxiliary block of ``rows`` rows handed to ``observe`` under that
          name (at most four different ones); option ``take=[row indices]`` picks rows, the default is all of them.

        Every term takes ``scale`` and ``offset`` (a scalar or one value per element, for instance the default pose): the
        element is ``(x - offset) * scale``.  A term is found in ``slices`` under its name (a source under its source
        name), or under the option ``key``.  ``out_dtype``: float32 or ``dtype`` (the default).  ``ValueError`` for an
        unknown term, option or joint, a key used twice, a row out of range, a value that is not finite in ``dtype``, more
        than four sources, no element at all or more than 4096."""
        lay = StateLayout.of(model)
        dt = np.dtype(dtype)
        _lib.dtype_code(dt)
        odt = dt if out_dtype is None else np.dtype(out_dtype)
        if odt not in (np.dtype(np.float32), dt):
            raise ValueError(f"out_dtype {odt}: expected float32 or {dt}")
        if velocity_representation is not None:
            velocity_representation = VelRepr(velocity_representation)
        slots, offset, scale, slices, src_names, src_rows = [], [], [], {}, [], []
        if isinstance(terms, (str, bytes)):
            raise ValueError("terms must be a sequence of names or (name, options), not one string")
        for term in terms:
            if isinstance(term, str):
                name, opts = term, {}
            elif isinstance(term, (tuple, list)) and len(term) == 2 and isinstance(term[0], str) and isinstance(term[1], dict):
                name, opts = term[0], dict(term[1])
            else:
                raise ValueError(f"term {term!r}: expected a name or (name, options)")
            key = opts.pop("key", None)
            t_scale, t_offset = opts.pop("scale", 1.0), opts.pop("offset", 0.0)
            mine, default_key = _term_slots(model, lay, term, name, opts, src_names, src_rows, "observation")
            key = default_key if key is None else key
            if opts:
                raise ValueError(f"term {name!r}: unknown options {sorted(opts)}")
            if key in slices:
                raise ValueError(f"two terms under the key {key!r}: give one of them the option key=")
            vals = [_per_element(name, what, v, len(mine), dt) for what, v in (("scale", t_scale), ("offset", t_offset))]
            slices[key] = slice(len(slots), len(slots) + len(mine))
            slots += mine
            scale += list(vals[0])
            offset += list(vals[1])
        if not 1 <= len(slots) <= OBS_MAX_WIDTH:
            raise ValueError(f"an observation of {len(slots)} elements: expected 1 .. {OBS_MAX_WIDTH}")
        return ObservationSpec(lay, dt, odt, velocity_representation, slots, offset, scale, slices, src_names, src_rows)

    _destroy = "jxs_observation_destroy"

    def _create(self, dm, handle) -> None:
        rows = (C.c_int32 * 4)(*(list(self.source_rows) + [0] * (4 - len(self.source_rows))))
        _lib.check(
            _lib.load().jxs_observation_create(
                dm.handle, self.size, self.slots.ctypes.data_as(C.POINTER(C.c_int32)), self.offset.ctypes.data_as(C.POINTER(C.c_double)),
                self.scale.ctypes.data_as(C.POINTER(C.c_double)), rows, C.byref(handle)),
            "jxs_observation_create",
        )  # fmt: skip


# modes of an action-table entry (JXS_ACT_* of include/jaxsim_amd.h) and the order of its eight parameters
ACT_OFF, ACT_TORQUE, ACT_POSITION, ACT_VELOCITY = range(4)
ACT_MODES = {"off": ACT_OFF, "torque": ACT_TORQUE, "position": ACT_POSITION, "velocity": ACT_VELOCITY}
ACT_PARAMS = ("scale", "offset", "kp", "kd", "action_clip", "target_lo", "target_hi", "torque_limit")
ACT_MAX_WIDTH = 4096


class ActionSpec(_SpecTable):
    """How ``JaxSimModelData.act`` turns a policy's action tensor into joint torques for one model: one entry per joint of
    the model, ``(mode, column)`` and the eight parameters ``ACT_PARAMS`` (the table of ``jxs_action_create``).  Built once on
    the host -- no device is needed --, uploaded at the first ``act``, used for every sub-step of a loop.

    ``joints`` ``[n, 2]`` int32, ``params`` ``[n, 8]`` float64, ``width``: the columns of the action tensor,
    ``joint_names``: the joints the policy drives, in column order, ``columns``: joint name -> column."""

    def __init__(self, layout: StateLayout, dtype, joints, params, width: int, joint_names):
        self.layout = layout
        self.dtype = np.dtype(dtype)
        self.joints = np.ascontiguousarray(joints, dtype=np.int32).reshape(-1, 2)
        self.params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 8)
        self.width = int(width)
        self.joint_names = tuple(joint_names)
        self.columns = {nm: c for c, nm in enumerate(self.joint_names)}

    @property
    def reads_actions(self) -> bool:
        return bool((self.joints[:, 1] >= 0).any())

    @staticmethod
    def build(model, *, dtype=np.float32, joints=None, mode="position", kp=0.0, kd=0.0, scale=1.0, offset=0.0, action_clip=np.inf,
              clip_to_position_limits=False, target_limits=None, torque_limit=np.inf, hold=None, hold_kp=None, hold_kd=None,
              width=None) -> "ActionSpec":  # fmt: skip
        """``joints`` names and orders the action columns (column ``c`` drives ``joints[c]``; the default is every joint, in
        model order).  Per named joint, with ``a`` its action word:

            u   = clamp(a, -action_clip, action_clip) * scale + offset
            tau = "torque"    u
                  "position"  kp * (clamp(u, target_lo, target_hi) - q) - kd * qdot
                  "velocity"  kd * (u - qdot)
                  "off"       0
            tau = clamp(tau [+ feed_forward], -torque_limit, torque_limit)

        ``mode`` and every numeric option is a scalar, one value per named joint, or a ``{joint name: value}`` dict (joints it
        leaves out keep the default).  ``target_limits=(lo, hi)``, each in one of these forms; ``clip_to_position_limits=True``
        takes the model's position limits instead.  ``hold={name: q}`` gives joints the policy does not drive a ``"position"``
        entry without a column that holds ``q`` with ``hold_kp`` / ``hold_kd`` (scalars or dicts over the held joints; the
        default is a scalar ``kp`` / ``kd``); a scalar or dict ``torque_limit`` applies to them too.  Joints neither named nor
        held are ``"off"``.  ``width``: the action tensor's column count, ``len(joints)`` by default.

        ``ValueError`` for an unknown joint or mode, a joint named twice or both named and held, a value that is not finite
        in ``dtype``, negative or NaN limits, ``lo > hi``, a width below ``len(joints)`` or above 4096, a model without joints."""
        lay = StateLayout.of(model)
        dt = np.dtype(dtype)
        _lib.dtype_code(dt)
        n = lay.n_joints
        if n < 1:
            raise ValueError("the model has no joints: there is nothing to actuate")
        names = list(model.joint_names())
        known = {nm: i for i, nm in enumerate(names)}
        named = list(names if joints is None else joints)
        if isinstance(joints, (str, bytes)):
            raise ValueError("joints must be a sequence of joint names, not one string")
        missing = [j for j in named if j not in known]
        if missing:
            raise ValueError(f"unknown joints {missing}")
        if len(set(named)) != len(named):
            raise ValueError("a joint is named twice")
        hold = dict(hold or {})
        missing = [j for j in hold if j not in known]
        if missing:
            raise ValueError(f"hold: unknown joints {missing}")
        both = [j for j in hold if j in named]
        if both:
            raise ValueError(f"joints {both} are both named and held")
        k = len(named)
        A = k if width is None else int(width)
        if A < k or A > ACT_MAX_WIDTH:
            raise ValueError(f"width {A}: expected {k} .. {ACT_MAX_WIDTH}")

        def per_joint(what, value, default, over, convert=float):
            """One value per joint of ``over`` from a scalar, a sequence or a {name: value} dict."""
            if isinstance(value, dict):
                unknown = [j for j in value if j not in over]
                if unknown:
                    raise ValueError(f"{what}: joints {unknown} are not among {list(over)}")
                return [convert(value.get(j, default)) for j in over]
            if isinstance(value, (str, bytes)) or np.ndim(value) == 0:
                return [convert(value)] * len(over)
            vals = list(value)
            if len(vals) != len(over):
                raise ValueError(f"{what}: {len(vals)} values for {len(over)} joints")
            return [convert(v) for v in vals]

        def mode_code(m):
            if isinstance(m, str) and m in ACT_MODES:
                return ACT_MODES[m]
            raise ValueError(f"unknown mode {m!r}: expected one of {sorted(ACT_MODES)}")

        if clip_to_position_limits and target_limits is not None:
            raise ValueError("give either clip_to_position_limits or target_limits")
        if target_limits is not None:
            if not isinstance(target_limits, (tuple, list)) or len(target_limits) != 2:
                raise ValueError("target_limits must be a pair (lo, hi)")
            t_lo, t_hi = target_limits
        elif clip_to_position_limits:
            kdp = model.kin_dyn_parameters
            lo_all, hi_all = np.asarray(kdp.position_limits_min, dtype=float), np.asarray(kdp.position_limits_max, dtype=float)
            t_lo, t_hi = [lo_all[known[j]] for j in named], [hi_all[known[j]] for j in named]
        else:
            t_lo, t_hi = -np.inf, np.inf
        cols = {
            "mode": per_joint("mode", mode, "position", named, mode_code),
            "scale": per_joint("scale", scale, 1.0, named), "offset": per_joint("offset", offset, 0.0, named),
            "kp": per_joint("kp", kp, 0.0, named), "kd": per_joint("kd", kd, 0.0, named),
            "action_clip": per_joint("action_clip", action_clip, np.inf, named),
            "target_lo": per_joint("target_limits[0]", t_lo, -np.inf, named), "target_hi": per_joint("target_limits[1]", t_hi, np.inf, named),
        }  # fmt: skip
        held = list(hold)
        everyone = named + held
        if isinstance(torque_limit, dict) or np.ndim(torque_limit) == 0:
            limits = per_joint("torque_limit", torque_limit, np.inf, everyone)
        else:
            limits = per_joint("torque_limit", torque_limit, np.inf, named) + [np.inf] * len(held)
        h_kp = h_kd = []
        if held:  # (without held joints the hold gains are not looked at: kp / kd may then have any of their forms)
            for what, own, general in (("hold_kp", hold_kp, kp), ("hold_kd", hold_kd, kd)):
                if own is None and (isinstance(general, dict) or np.ndim(general) != 0):
                    raise ValueError(f"{what} is needed: {what[5:]} is not a scalar")
            h_kp = per_joint("hold_kp", kp if hold_kp is None else hold_kp, 0.0, held)
            h_kd = per_joint("hold_kd", kd if hold_kd is None else hold_kd, 0.0, held)
        table = np.full((n, 2), (ACT_OFF, -1), dtype=np.int32)
        params = np.tile(np.array([1.0, 0.0, 0.0, 0.0, np.inf, -np.inf, np.inf, np.inf]), (n, 1))
        for c, j in enumerate(named):
            table[known[j]] = (cols["mode"][c], c)
            params[known[j]] = [cols[p][c] for p in ACT_PARAMS[:-1]] + [limits[c]]
        for i, j in enumerate(held):
            table[known[j]] = (ACT_POSITION, -1)
            params[known[j]] = [1.0, float(hold[j]), h_kp[i], h_kd[i], np.inf, -np.inf, np.inf, limits[k + i]]

        def finite(v):
            with np.errstate(over="ignore"):
                return bool(np.isfinite(v) and np.isfinite(np.float64(v).astype(dt)))

        for i in range(n):
            p = dict(zip(ACT_PARAMS, params[i]))
            for what in ("scale", "offset", "kp", "kd"):
                if not finite(p[what]):
                    raise ValueError(f"joint {names[i]!r}: {what} = {p[what]} is not finite in {dt.name}")
            for what in ("action_clip", "torque_limit"):
                if not (p[what] >= 0 and (np.isposinf(p[what]) or finite(p[what]))):
                    raise ValueError(f"joint {names[i]!r}: {what} = {p[what]}: expected a value >= 0 that is finite in {dt.name}, or +inf")
            lo, hi = p["target_lo"], p["target_hi"]
            if not (lo <= hi and all(np.isinf(v) or finite(v) for v in (lo, hi))):
                raise ValueError(f"joint {names[i]!r}: target limits ({lo}, {hi}): expected lo <= hi, each infinite or finite in {dt.name}")
        return ActionSpec(lay, dt, table, params, A, named)

    _destroy = "jxs_action_destroy"

    def _create(self, dm, handle) -> None:
        _lib.check(
            _lib.load().jxs_action_create(dm.handle, self.width, self.joints.ctypes.data_as(C.POINTER(C.c_int32)),
                                          self.params.ctypes.data_as(C.POINTER(C.c_double)), C.byref(handle)),
            "jxs_action_create",
        )  # fmt: skip


# inners, outers and condition kinds of an evaluation table (JXS_EVAL_* of include/jaxsim_amd.h), the bits of the done byte
EVAL_INNERS = {"identity": 0, "abs": 1, "square": 2, "excess": 3}
EVAL_OUTERS = {"identity": 0, "exp": 1}
EVAL_KINDS = {"terminated": 0, "truncated": 1}
EVAL_MAX_SLOTS, EVAL_MAX_TERMS, EVAL_MAX_CONDITIONS = 1024, 32, 32
DONE_TERMINATED, DONE_TRUNCATED = 1, 2


class RewardSpec(_SpecTable):
    """What ``JaxSimModelData.evaluate`` computes for one model: named reward terms and termination conditions over slots
    ``(kind, source, index)`` with an offset, a scale and optionally a target each (the table of ``jxs_evaluation_create``).
    Built once on the host -- no device is needed --, uploaded at the first ``evaluate``, used for every step of a loop.

    ``slots`` ``[D, 3]`` / ``targets`` ``[D, 2]`` int32, ``offset`` / ``scale`` ``[D]`` float64, ``terms`` ``[K, 4]`` int32 =
    first, count, inner, outer with ``term_params`` ``[K, 3]`` = weight, lo, hi, ``conditions`` ``[C, 2]`` int32 = slot, kind with
    ``condition_limits`` ``[C, 2]`` = lo, hi.  ``term_names`` name the columns of ``evaluate(terms=)``, ``condition_names`` the
    bits of ``evaluate(fired=)``, ``names`` is both; ``source_names`` / ``source_rows``: the blocks ``evaluate`` must be given."""

    def __init__(self, layout: StateLayout, dtype, velocity_representation, slots, targets, offset, scale, terms, term_params, conditions,
                 condition_limits, reward_clip, termination_reward, term_names, condition_names, source_names, source_rows):  # fmt: skip
        self.layout = layout
        self.dtype = np.dtype(dtype)
        self.velocity_representation = None if velocity_representation is None else VelRepr(velocity_representation)
        self.slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1, 3)
        self.targets = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1, 2)
        self.offset = np.ascontiguousarray(offset, dtype=np.float64)
        self.scale = np.ascontiguousarray(scale, dtype=np.float64)
        self.terms = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1, 4)
        self.term_params = np.ascontiguousarray(term_params, dtype=np.float64).reshape(-1, 3)
        self.conditions = np.ascontiguousarray(conditions, dtype=np.int32).reshape(-1, 2)
        self.condition_limits = np.ascontiguousarray(condition_limits, dtype=np.float64).reshape(-1, 2)
        self.reward_clip = (float(reward_clip[0]), float(reward_clip[1]))
        self.termination_reward = float(termination_reward)
        self.term_names, self.condition_names = tuple(term_names), tuple(condition_names)
        self.names = self.term_names + self.condition_names
        self.source_names, self.source_rows = tuple(source_names), tuple(int(r) for r in source_rows)

    @property
    def n_terms(self) -> int:
        return self.terms.shape[0]

    @property
    def n_conditions(self) -> int:
        return self.conditions.shape[0]

    @staticmethod
    def build(model, rewards=(), terminations=(), *, reward_clip=(-np.inf, np.inf), termination_reward=0.0, dtype=np.float32,
              velocity_representation=None) -> "RewardSpec":  # fmt: skip
        """``rewards``: an ordered sequence of ``(name, options)``, at most 32.  ``term=`` names what the term reads, by the names
        of ``ObservationSpec.build`` (``"joint_positions"`` / ``"joint_velocities"`` with ``joints=[names]``, ``"base_height"``,
        ``"projected_gravity"``, ``"base_velocity"`` ..., or ``("source", dict(name=, rows=, take=))``); ``index=`` (an int or a
        list) picks elements of it; ``offset=`` and ``scale=`` are a scalar or one value per element.  With ``y = (x - offset) *
        scale`` of every element the term contributes

            clip(weight * outer(sum inner(y)), *clip)

        ``inner``: ``"identity"``, ``"abs"``, ``"square"`` or ``"excess"`` (``max(|y| - 1, 0)``); ``outer``: ``"identity"`` or
        ``"exp"`` (``exp(-sum)``); ``weight`` defaults to 1, ``clip=(lo, hi)`` to no limits.  ``sigma`` divides the scales -- for
        ``"square"`` by ``sqrt(sigma)``, so that ``outer="exp"`` gives ``exp(-sum (d / sqrt(sigma))^2)``.  ``target=("source",
        dict(name=, rows=, row=))`` subtracts row ``row`` (an int, or one per element) of a source block from ``x`` first: the
        commanded value of the environment.  ``inner="excess"`` on ``"joint_positions"`` without ``offset`` and ``scale`` takes
        the model's position limits (``ActionSpec``'s ``clip_to_position_limits``): the term is how far, in half-ranges, each
        joint lies outside them.

        ``terminations``: ``(name, dict(term=, index=, offset=, scale=, target=, below=, above=, kind=))``, at most 32 elements
        in all: the condition fires when ``y < below`` or ``y > above`` or ``y`` is NaN and sets ``kind`` (``"terminated"``, the
        default, or ``"truncated"``) in the done byte.  A term of several elements gives one condition per element, named
        ``name[i]``.

        The reward is ``clip(sum of the terms, *reward_clip)``, plus ``termination_reward`` where a ``"terminated"`` condition
        fired.  ``ValueError`` for an unknown term, option, joint, inner, outer or kind, a name used twice, a value that is not
        finite in ``dtype``, ``lo > hi``, a ``sigma`` that is not positive, infinite joint limits, more than four sources, no
        element at all or more than 1024."""
        lay = StateLayout.of(model)
        dt = np.dtype(dtype)
        _lib.dtype_code(dt)
        if velocity_representation is not None:
            velocity_representation = VelRepr(velocity_representation)
        src_names, src_rows = [], []
        slots, targets, offset, scale = [], [], [], []

        def finite(v) -> bool:
            with np.errstate(over="ignore"):
                return bool(np.isfinite(v) and np.isfinite(np.float64(v).astype(dt)))

        def limits(name, what, pair):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"{name!r}: {what} must be a pair (lo, hi)")
            lo, hi = float(pair[0]), float(pair[1])
            if not (lo <= hi and all(np.isinf(v) or finite(v) for v in (lo, hi))):
                raise ValueError(f"{name!r}: {what} = ({lo}, {hi}): expected lo <= hi, each infinite or finite in {dt.name}")
            return lo, hi

        def entries(what, seq):
            if isinstance(seq, (str, bytes, dict)):
                raise ValueError(f"{what} must be a sequence of (name, options)")
            seen = []
            for item in seq:
                if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], str) and isinstance(item[1], dict)):
                    raise ValueError(f"{what}: {item!r}: expected (name, options)")
                seen.append((item[0], dict(item[1])))
            return seen

        def elements(name, opts, inner=None):
            """The slots of an entry with their offset, scale and target; the options used are taken out of ``opts``."""
            term = opts.pop("term", None)
            if isinstance(term, str):
                tname, topts = term, {}
            elif isinstance(term, (tuple, list)) and len(term) == 2 and isinstance(term[0], str) and isinstance(term[1], dict):
                tname, topts = term[0], dict(term[1])
            else:
                raise ValueError(f"{name!r}: term = {term!r}: expected a name or (name, options)")
            if "joints" in opts:
                topts["joints"] = opts.pop("joints")
            mine, _ = _term_slots(model, lay, term, tname, topts, src_names, src_rows, "reward")
            if topts:
                raise ValueError(f"{name!r}: term {tname!r}: unknown options {sorted(topts)}")
            index = opts.pop("index", None)
            if index is not None:
                picks = [int(index)] if np.ndim(index) == 0 else [int(i) for i in index]
                if any(i < 0 or i >= len(mine) for i in picks):
                    raise ValueError(f"{name!r}: index {picks} outside [0, {len(mine)})")
                mine = [mine[i] for i in picks]
            if not mine:
                raise ValueError(f"{name!r}: the term has no element")
            t_offset, t_scale = opts.pop("offset", None), opts.pop("scale", None)
            if inner == "excess" and tname == "joint_positions" and t_offset is None and t_scale is None:
                kdp = model.kin_dyn_parameters
                lo_all, hi_all = np.asarray(kdp.position_limits_min, dtype=float), np.asarray(kdp.position_limits_max, dtype=float)
                j = [s[2] - lay.row_s for s in mine]
                lo, hi = lo_all[j], hi_all[j]
                if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
                    raise ValueError(f"{name!r}: the position limits of some named joint are infinite or empty")
                t_offset, t_scale = (lo + hi) / 2, 2.0 / (hi - lo)
            sc = _per_element(name, "scale", 1.0 if t_scale is None else t_scale, len(mine), dt)
            off = _per_element(name, "offset", 0.0 if t_offset is None else t_offset, len(mine), dt)
            tg = opts.pop("target", None)
            mine_targets = [(-1, 0)] * len(mine)
            if tg is not None:
                if not (isinstance(tg, (tuple, list)) and len(tg) == 2 and tg[0] == "source" and isinstance(tg[1], dict)):
                    raise ValueError(f"{name!r}: target = {tg!r}: expected ('source', dict(name=, rows=, row=))")
                gopts = dict(tg[1])
                row = gopts.pop("row", None)
                if row is None:
                    raise ValueError(f"{name!r}: a target needs row=")
                rows_of = [int(row)] * len(mine) if np.ndim(row) == 0 else [int(r) for r in row]
                if len(rows_of) != len(mine):
                    raise ValueError(f"{name!r}: {len(rows_of)} target rows for {len(mine)} elements")
                gopts["take"] = rows_of
                got, _ = _term_slots(model, lay, tg, "source", gopts, src_names, src_rows, "reward")
                if gopts:
                    raise ValueError(f"{name!r}: target: unknown options {sorted(gopts)}")
                mine_targets = [(s, r) for _, s, r in got]
            return mine, off, sc, mine_targets

        def choice(name, what, value, table):
            if not isinstance(value, str) or value not in table:
                raise ValueError(f"{name!r}: unknown {what} {value!r}: expected one of {sorted(table)}")
            return table[value]

        terms, term_params, term_names = [], [], []
        for name, opts in entries("rewards", rewards):
            inner_name, outer_name = opts.pop("inner", "identity"), opts.pop("outer", "identity")
            inner, outer = choice(name, "inner", inner_name, EVAL_INNERS), choice(name, "outer", outer_name, EVAL_OUTERS)
            mine, off, sc, tg = elements(name, opts, inner_name)
            sigma = opts.pop("sigma", None)
            if sigma is not None:
                sigma = float(sigma)
                if not (sigma > 0 and np.isfinite(sigma)):
                    raise ValueError(f"{name!r}: sigma = {sigma}: expected a positive number")
                sc = _per_element(name, "scale / sigma", sc / (np.sqrt(sigma) if inner_name == "square" else sigma), len(mine), dt)
            weight = float(opts.pop("weight", 1.0))
            if not finite(weight):
                raise ValueError(f"{name!r}: weight = {weight} is not finite in {dt.name}")
            lo, hi = limits(name, "clip", opts.pop("clip", (-np.inf, np.inf)))
            if opts:
                raise ValueError(f"{name!r}: unknown options {sorted(opts)}")
            terms.append((len(slots), len(mine), inner, outer))
            term_params.append((weight, lo, hi))
            term_names.append(name)
            slots += mine
            targets += tg
            offset += list(off)
            scale += list(sc)
        conditions, condition_limits, condition_names = [], [], []
        for name, opts in entries("terminations", terminations):
            kind = choice(name, "kind", opts.pop("kind", "terminated"), EVAL_KINDS)
            mine, off, sc, tg = elements(name, opts)
            lo, hi = limits(name, "(below, above)", (opts.pop("below", -np.inf), opts.pop("above", np.inf)))
            if opts:
                raise ValueError(f"{name!r}: unknown options {sorted(opts)}")
            for i in range(len(mine)):
                conditions.append((len(slots) + i, kind))
                condition_limits.append((lo, hi))
                condition_names.append(name if len(mine) == 1 else f"{name}[{i}]")
            slots += mine
            targets += tg
            offset += list(off)
            scale += list(sc)
        names = term_names + condition_names
        if len(set(names)) != len(names):
            raise ValueError("a name is used twice")
        if len(terms) > EVAL_MAX_TERMS or len(conditions) > EVAL_MAX_CONDITIONS:
            raise ValueError(f"{len(terms)} terms and {len(conditions)} conditions: at most {EVAL_MAX_TERMS} and {EVAL_MAX_CONDITIONS}")
        if not 1 <= len(slots) <= EVAL_MAX_SLOTS:
            raise ValueError(f"a table of {len(slots)} elements: expected 1 .. {EVAL_MAX_SLOTS}")
        clip = limits("reward_clip", "reward_clip", reward_clip)
        if not finite(termination_reward):
            raise ValueError(f"termination_reward = {termination_reward} is not finite in {dt.name}")
        return RewardSpec(lay, dt, velocity_representation, slots, targets, offset, scale, terms, term_params, conditions, condition_limits, clip,
                          termination_reward, term_names, condition_names, src_names, src_rows)  # fmt: skip

    _destroy = "jxs_evaluation_destroy"

    def _desc(self):
        """The ``jxs_evaluation_desc`` of this spec; its pointers are into this object's arrays."""
        d = _lib.EvaluationDesc()
        d.D, d.K, d.C = self.slots.shape[0], self.n_terms, self.n_conditions
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        d.slots, d.targets = self.slots.ctypes.data_as(i32), self.targets.ctypes.data_as(i32)
        d.offset, d.scale = self.offset.ctypes.data_as(f64), self.scale.ctypes.data_as(f64)
        d.terms, d.term_params = self.terms.ctypes.data_as(i32), self.term_params.ctypes.data_as(f64)
        d.conditions, d.condition_limits = self.conditions.ctypes.data_as(i32), self.condition_limits.ctypes.data_as(f64)
        d.reward_lo, d.reward_hi = self.reward_clip
        d.termination_reward = self.termination_reward
        d.source_rows = (C.c_int32 * 4)(*(list(self.source_rows) + [0] * (4 - len(self.source_rows))))
        return d

    def _create(self, dm, handle) -> None:
        _lib.check(_lib.load().jxs_evaluation_create(dm.handle, C.byref(self._desc()), C.byref(handle)), "jxs_evaluation_create")


# rows of a group in the record of ``contact_sensors`` (JXS_CONTACT_* of include/jaxsim_amd.h), and the limits of a table
CONTACT_FIELDS = {"flag": 0, "count": 1, "clearance": 2, "slip_sq": 3, "air_time": 4, "contact_time": 5, "touchdown": 6, "flight_time": 7}
CONTACT_ROWS, CONTACT_TIMER_ROWS = 8, 2
CONTACT_MAX_POINTS, CONTACT_MAX_GROUPS = 1024, 32


class ContactSensorSpec(_SpecTable):
    """What ``JaxSimModelData.contact_sensors`` senses for one model: named groups of points on links (the table of
    ``jxs_contact_sensors_create``).  Built once on the host -- no device is needed --, uploaded at the first
    ``contact_sensors``, used for every step of a loop.

    ``groups`` ``[G, 2]`` int32 = first, count; ``parent`` ``[P]`` int32, the link of each entry; ``L_p`` ``[P, 3]`` float64, its
    position in the link frame; ``group_names`` name the groups, group ``g`` owning rows ``8 g + CONTACT_FIELDS[...]`` of the
    record and rows ``2 g``, ``2 g + 1`` of the timers."""

    def __init__(self, layout: StateLayout, dtype, n_links: int, group_names, groups, parent, L_p, model=None):
        self.layout = layout
        self._model = model  # (new_timers asks its device model for the tile)
        self.dtype = np.dtype(dtype)
        self.n_links = int(n_links)
        self.group_names = tuple(group_names)
        self.groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1, 2)
        self.parent = np.ascontiguousarray(parent, dtype=np.int32)
        self.L_p = np.ascontiguousarray(L_p, dtype=np.float64).reshape(-1, 3)

    @property
    def n_groups(self) -> int:
        return self.groups.shape[0]

    @property
    def n_rows(self) -> int:
        return CONTACT_ROWS * self.n_groups

    @property
    def n_timer_rows(self) -> int:
        return CONTACT_TIMER_ROWS * self.n_groups

    @staticmethod
    def build(model, groups, *, dtype=np.float32) -> "ContactSensorSpec":
        """``groups``: an ordered ``{name: dict(links=[link names])}`` -- the enabled collidable points of those links, in the
        order of the model -- or ``{name: dict(points=[(link name, xyz), ...])}`` -- explicit points, so that a model without
        collision shapes can be sensed too.  A point wanted in two groups is listed in both.  ``ValueError`` for an unknown
        link, an empty group, more than ``CONTACT_MAX_GROUPS`` groups or ``CONTACT_MAX_POINTS`` points, a point that is not
        finite in ``dtype``."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"dtype {dt} is not float32 or float64")
        if not isinstance(groups, dict) or not groups:
            raise ValueError("groups must be a non-empty dict {name: dict(links=[...]) or dict(points=[...])}")
        names = list(model.link_names())
        kdp = model.kin_dyn_parameters
        enabled = np.asarray(kdp.indices_of_enabled_collidable_points, dtype=np.int64)
        body, point = np.asarray(kdp.contact_body)[enabled], np.asarray(kdp.contact_point, dtype=np.float64).reshape(-1, 3)[enabled]
        table, parent, L_p = [], [], []
        for name, opts in groups.items():
            if not isinstance(opts, dict) or set(opts) not in ({"links"}, {"points"}):
                raise ValueError(f"group {name!r}: expected dict(links=[...]) or dict(points=[...]), not {opts!r}")
            first = len(parent)
            if "links" in opts:
                for link in opts["links"]:
                    if link not in names:
                        raise ValueError(f"group {name!r}: unknown link {link!r}")
                    on = np.flatnonzero(body == names.index(link))
                    parent += [names.index(link)] * len(on)
                    L_p += [point[k] for k in on]
            else:
                for entry in opts["points"]:
                    link, xyz = entry
                    if link not in names:
                        raise ValueError(f"group {name!r}: unknown link {link!r}")
                    xyz = np.asarray(xyz, dtype=np.float64)
                    if xyz.shape != (3,):
                        raise ValueError(f"group {name!r}: a point of link {link!r} of shape {xyz.shape}, not (3,)")
                    parent.append(names.index(link))
                    L_p.append(xyz)
            if len(parent) == first:
                raise ValueError(f"group {name!r} is empty: its links have no enabled collidable point")
            table.append((first, len(parent) - first))
        if len(table) > CONTACT_MAX_GROUPS or len(parent) > CONTACT_MAX_POINTS:
            raise ValueError(f"{len(table)} groups of {len(parent)} points: at most {CONTACT_MAX_GROUPS} groups and {CONTACT_MAX_POINTS} points")
        L_p = np.asarray(L_p, dtype=np.float64).reshape(-1, 3)
        with np.errstate(over="ignore"):
            if not (np.isfinite(L_p).all() and np.isfinite(L_p.astype(dt)).all()):
                raise ValueError(f"a point is not finite in {dt.name}")
        return ContactSensorSpec(StateLayout.of(model), dt, model.number_of_links(), groups.keys(), table, parent, L_p, model)

    def rows(self, group, field) -> list[int]:
        """Row numbers of the record: of one group or a list of groups (``None``: all), one field or a list of fields of
        ``CONTACT_FIELDS``, group-major."""
        gs = list(self.group_names) if group is None else [group] if isinstance(group, str) else list(group)
        fs = [field] if isinstance(field, str) else list(field)
        unknown = [g for g in gs if g not in self.group_names] + [f for f in fs if f not in CONTACT_FIELDS]
        if unknown:
            raise ValueError(f"unknown groups or fields {unknown}: groups {list(self.group_names)}, fields {list(CONTACT_FIELDS)}")
        return [CONTACT_ROWS * self.group_names.index(g) + CONTACT_FIELDS[f] for g in gs for f in fs]

    def source(self, name: str, fields, groups=None):
        """The term ``("source", dict(name=, rows=, take=))`` of ``ObservationSpec.build`` and ``RewardSpec.build`` that reads
        ``fields`` of ``groups`` (``None``: all) from the record passed to ``observe`` / ``evaluate`` as ``sources={name: record}``."""
        return ("source", dict(name=name, rows=self.n_rows, take=self.rows(groups, fields)))

    def new_timers(self, N: int, *, tile: int | None = None) -> runtime.DeviceArray:
        """A zeroed timer block ``[2 G][N]`` for ``contact_sensors(timers=)``, in the tiling of the spec's model (``tile``:
        another one)."""
        if tile is None:
            if self._model is None:
                raise ValueError("a spec that was not built from a model needs tile=")
            tile = runtime.device_model(self._model, self.dtype).layout.tile
        return runtime.DeviceArray(self.n_timer_rows, int(N), self.dtype, tile=tile, zero=True)

    _destroy = "jxs_contact_sensors_destroy"

    def _create(self, dm, handle) -> None:
        i32 = C.POINTER(C.c_int32)
        _lib.check(
            _lib.load().jxs_contact_sensors_create(dm.handle, self.n_groups, self.groups.ctypes.data_as(i32), len(self.parent), self.parent.ctypes.data_as(i32),
                                                   self.L_p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(handle)),
            "jxs_contact_sensors_create",
        )  # fmt: skip
