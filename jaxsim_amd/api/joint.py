"""``jaxsim.api.joint`` mirror (``src/jaxsim/api/joint.py``): joint names, indices and position limits.

Joint ``j`` moves link ``j + 1``.  ``random_joint_positions`` samples inside the joint limits by the reference's rule
(a revolute joint of range >= 2 pi is sampled from a window of 2 pi) from the counter-based generator of the device
(Philox4x32-10, ``csrc/jxs_env_random.h``), not from JAX's threefry streams, which cannot be reproduced here: it returns
the joint positions ``JaxSimModelData.reset_random_where`` draws for environment 0 with the same ``seed`` and ``draw``.
"""

from __future__ import annotations

import numpy as np

from .. import _philox

REVOLUTE = 1  # kin_dyn_parameters.joint_types


def _check(model, joint_index) -> int:
    i = int(joint_index)
    if i < 0 or i >= model.number_of_joints():
        raise ValueError(f"Invalid joint index '{i}'")
    return i


def name_to_idx(model, *, joint_name: str) -> int:
    """``name_to_idx`` (joint.py:18-41)."""
    names = model.joint_names()
    if joint_name not in names:
        raise ValueError(f"Joint '{joint_name}' not found in the model")
    return names.index(joint_name)


def idx_to_name(model, *, joint_index) -> str:
    """``idx_to_name`` (joint.py:44-64)."""
    return model.joint_names()[_check(model, joint_index)]


def names_to_idxs(model, *, joint_names) -> np.ndarray:
    """``names_to_idxs`` (joint.py:67-83)."""
    return np.array([name_to_idx(model, joint_name=nm) for nm in joint_names], dtype=int)


def idxs_to_names(model, *, joint_indices) -> tuple[str, ...]:
    """``idxs_to_names`` (joint.py:86-104)."""
    return tuple(idx_to_name(model, joint_index=i) for i in np.asarray(joint_indices).reshape(-1))


def position_limit(model, *, joint_index) -> tuple[float, float]:
    """``position_limit`` (joint.py:111-145): ``(s_min, s_max)`` of one joint."""
    if model.number_of_joints() == 0:
        return np.empty(0), np.empty(0)
    j = _check(model, joint_index)
    kdp = model.kin_dyn_parameters
    return float(kdp.position_limits_min[j]), float(kdp.position_limits_max[j])


def position_limits(model, *, joint_names=None) -> tuple[np.ndarray, np.ndarray]:
    """``position_limits`` (joint.py:148-181): ``(s_min, s_max)`` of the named joints, of all joints by default."""
    idx = names_to_idxs(model, joint_names=joint_names) if joint_names is not None else np.arange(model.number_of_joints())
    if len(idx) == 0:
        return np.empty(0), np.empty(0)
    kdp = model.kin_dyn_parameters
    return np.asarray(kdp.position_limits_min, dtype=float)[idx], np.asarray(kdp.position_limits_max, dtype=float)[idx]


def random_position_window(s_min, s_max, revolute) -> tuple[np.ndarray, np.ndarray]:
    """The interval joint positions are sampled from, given the position limits and which joints are revolute: the rule
    of the reference's ``random_joint_positions`` (joint.py:209-267).  A revolute joint whose range is 2 pi or more (a
    continuous joint) is sampled from a window of 2 pi: ``[-pi, pi]`` when the limits contain it, else the window that
    ends at an upper limit below pi, else the one that starts at a lower limit above -pi.  Other joints keep their limits."""
    s_min, s_max = np.array(s_min, dtype=float).reshape(-1), np.array(s_max, dtype=float).reshape(-1)
    revolute = np.asarray(revolute, dtype=bool).reshape(-1)
    pi = np.pi
    with np.errstate(over="ignore", invalid="ignore"):
        full = revolute & (s_max - s_min >= 2 * pi)
        s_min = np.where(full & (s_min <= -pi) & (s_max >= pi), -pi, s_min)
        s_max = np.where(full & (s_min <= -pi) & (s_max >= pi), pi, s_max)
        s_min = np.where(full & (s_max < pi), s_max - 2 * pi, s_min)
        s_max = np.where(full & (s_min > -pi), s_min + 2 * pi, s_max)
    return s_min, s_max


def random_position_bounds(model, *, joint_names=None, dtype=np.float64) -> tuple[np.ndarray, np.ndarray]:
    """``(lo, hi)`` in ``dtype`` of the named joints (all by default) by ``random_position_window``.  ``ValueError`` when
    a bound, or the width ``hi - lo``, is not finite in ``dtype`` (a prismatic joint without limits): the reference
    would sample NaN there."""
    idx = names_to_idxs(model, joint_names=joint_names) if joint_names is not None else np.arange(model.number_of_joints())
    lo, hi = position_limits(model, joint_names=joint_names)
    revolute = np.asarray(model.kin_dyn_parameters.joint_types)[idx] == REVOLUTE if len(idx) else np.zeros(0, dtype=bool)
    lo, hi = random_position_window(lo, hi, revolute)
    with np.errstate(over="ignore", invalid="ignore"):
        lo, hi = lo.astype(dtype), hi.astype(dtype)
        bad = ~(np.isfinite(lo) & np.isfinite(hi) & np.isfinite(hi - lo))
    if bad.any():
        names = [model.joint_names()[int(i)] for i in np.asarray(idx)[bad]]
        raise ValueError(f"joints {names} have no finite position range in {np.dtype(dtype).name}: pass explicit joint_pos_bounds")
    return lo, hi


def random_joint_positions(model, *, joint_names=None, seed: int = 0, draw: int = 0) -> np.ndarray:
    """``random_joint_positions`` (joint.py:184-281) in float64 on the host: uniform inside ``random_position_bounds``.
    Bit for bit the joint positions the device draws for (global) environment 0 of a float64 batch with the same
    ``seed`` and ``draw`` and the default joint bounds: joint ``j`` is variable ``6 + j`` of the sampler."""
    idx = names_to_idxs(model, joint_names=joint_names) if joint_names is not None else np.arange(model.number_of_joints())
    if len(idx) == 0:
        return np.empty(0)
    lo, hi = random_position_bounds(model, joint_names=joint_names)
    return _philox.uniform(lo, hi, 0, 6 + np.asarray(idx, dtype=np.uint64), seed, draw)
