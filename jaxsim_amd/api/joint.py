"""``jaxsim.api.joint`` mirror (``src/jaxsim/api/joint.py``): joint names, indices and position limits.

Joint ``j`` moves link ``j + 1``.  ``random_joint_positions`` is not provided: the reference draws from JAX's PRNG,
whose streams cannot be reproduced here.
"""

from __future__ import annotations

import numpy as np


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
