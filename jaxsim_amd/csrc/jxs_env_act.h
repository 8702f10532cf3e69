// The joint torques of one environment from a policy's action as plain functions (jxs_env_act in jxs_api.hip): the tiled
// [n][N] block jxs_step consumes, computed from an environment-major action tensor [N][act_ld] and the joint positions
// and velocities of the tiled state block.  Plain functions for host and device, no HIP types.  torque_word() is one
// word of the block; tests/emul/jxs_emul_env_act.cpp drives it over every word on the CPU, the kernel calls it once per
// word it stores.
//
// A table has one entry per joint j (0 .. n-1, the order of the state's joint rows): {mode, column} and the eight
// parameters kScale .. kTorqueLimit in the block's type T.  With clamp(x, lo, hi) = x < lo ? lo : (hi < x ? hi : x) -- a
// NaN x passes through, -0 keeps its sign, infinite bounds need no special case -- the word of joint j of environment e is
//   a   = column < 0 ? 0 : T(actions[e][column])                       (fp32 -> fp64 widening is exact)
//   u   = clamp(a, -action_clip, action_clip) * scale + offset         (the product rounded, then the sum)
//   t   = kOff 0 | kTorque u | kPosition kp * (clamp(u, target_lo, target_hi) - q_j) - kd * qd_j | kVelocity kd * (u - qd_j)
//   t   = feed_forward ? t + ff[j][e] : t
//   tau = clamp(t, -torque_limit, torque_limit)
// kPosition with column -1 holds `offset`: how joints the policy does not drive are kept stiff.
//
// Arithmetic is done in the block's type and every operation is rounded on its own (jxs_env_random.h: contraction off for
// hipcc and g++).  Only + - x and comparisons are involved, so host and device give the same bits.
#pragma once

#include <cstdint>

#include "jxs_env_observe.h"
#include "jxs_env_ops.h"
#include "jxs_env_random.h"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace jxs_act {

constexpr int kMaxWidth = 4096;  // JXS_ACT_MAX_WIDTH of include/jaxsim_amd.h
// JXS_ACT_* of include/jaxsim_amd.h
constexpr int kOff = 0, kTorque = 1, kPosition = 2, kVelocity = 3;
constexpr int kModes = 4;
// the parameters of a joint, in the order of `params` [n][8]
constexpr int kScale = 0, kOffset = 1, kKp = 2, kKd = 3, kActionClip = 4, kTargetLo = 5, kTargetHi = 6, kTorqueLimit = 7;
constexpr int kParams = 8;

// rows of the joint positions and velocities in the state block (jaxsim_amd/state.py)
JXS_ENV_HD int row_q(int) { return 7; }
JXS_ENV_HD int row_qd(int n_joints) { return 13 + n_joints; }

template <typename T>
JXS_ENV_HD T clamp(T x, T lo, T hi) {
  return x < lo ? lo : (hi < x ? hi : x);
}

// u of a joint: the clipped action, scaled and shifted; two roundings
template <typename T>
JXS_ENV_HD T target(T a, T action_clip, T scale, T offset) {
  JXS_RAND_NO_CONTRACT
  const T p = clamp(a, -action_clip, action_clip) * scale;
  return p + offset;
}

// t of a joint before the feed-forward term and the torque limit
template <typename T>
JXS_ENV_HD T mode_torque(int mode, T u, T kp, T kd, T target_lo, T target_hi, T q, T qd) {
  JXS_RAND_NO_CONTRACT
  if (mode == kTorque) return u;
  if (mode == kPosition) {
    const T d = clamp(u, target_lo, target_hi) - q;
    const T p = kp * d;
    const T v = kd * qd;
    return p - v;
  }
  if (mode == kVelocity) {
    const T d = u - qd;
    return kd * d;
  }
  return T(0);
}

template <typename T>
JXS_ENV_HD T limited(T t, bool feed_forward, T ff, T torque_limit) {
  JXS_RAND_NO_CONTRACT
  const T s = feed_forward ? t + ff : t;
  return clamp(s, -torque_limit, torque_limit);
}

// The word of a joint of an environment: `a` is the action word of its column (ignored for column < 0), p its eight parameters
template <typename T>
JXS_ENV_HD T torque_word(int mode, int column, T a, const T p[kParams], T q, T qd, bool feed_forward, T ff) {
  const T u = target(column < 0 ? T(0) : a, p[kActionClip], p[kScale], p[kOffset]);
  return limited(mode_torque(mode, u, p[kKp], p[kKd], p[kTargetLo], p[kTargetHi], q, qd), feed_forward, ff, p[kTorqueLimit]);
}

// scale, offset, kp, kd must be finite in the block's type
JXS_ENV_HD bool finite_ok(double v, float t) { return jxs_obs::affine_ok(v, t); }
JXS_ENV_HD bool finite_ok(double v, double t) { return jxs_obs::affine_ok(v, t); }
// an action clip or a torque limit: +inf, or >= 0 and finite in the block's type; never NaN
template <typename T>
JXS_ENV_HD bool limit_ok(double v, T t) {
  if (!(v >= 0.0)) return false;
  return v - v != 0.0 || finite_ok(v, t);
}
// target_lo <= target_hi; each infinite or finite in the block's type; no NaN
template <typename T>
JXS_ENV_HD bool targets_ok(double lo, double hi, T t) {
  if (!(lo <= hi)) return false;
  return (lo - lo != 0.0 || finite_ok(lo, t)) && (hi - hi != 0.0 || finite_ok(hi, t));
}

// Validity of a table: `joints` is [n][2] = {mode, column}, `params` [n][8], A the width of the action tensor
constexpr int kOk = 0, kBadJoints = 1, kBadWidth = 2, kBadMode = 3, kBadColumn = 4, kNotFinite = 5, kBadLimit = 6, kBadTargets = 7;
// kOk, or the first error and the joint it is in (-1: the table as a whole)
template <typename T>
JXS_ENV_HD int table_error(const int32_t* joints, const double* params, long long n, long long A, T t, int* bad_joint) {
  *bad_joint = -1;
  if (n < 1 || joints == nullptr || params == nullptr) return kBadJoints;
  if (A < 0 || A > kMaxWidth) return kBadWidth;
  for (int j = 0; j < (int)n; ++j) {
    const int mode = joints[2 * j], column = joints[2 * j + 1];
    const double* p = params + (long long)kParams * j;
    *bad_joint = j;
    if (mode < 0 || mode >= kModes) return kBadMode;
    if (column < -1 || column >= A) return kBadColumn;
    if (!finite_ok(p[kScale], t) || !finite_ok(p[kOffset], t) || !finite_ok(p[kKp], t) || !finite_ok(p[kKd], t)) return kNotFinite;
    if (!limit_ok(p[kActionClip], t) || !limit_ok(p[kTorqueLimit], t)) return kBadLimit;
    if (!targets_ok(p[kTargetLo], p[kTargetHi], t)) return kBadTargets;
  }
  *bad_joint = -1;
  return kOk;
}

// The table as the kernel reads it: per joint one word, mode | (column + 1) << 2, and its eight parameters in the block's
// type as one aligned record (two or four 16-byte loads)
JXS_ENV_HD int32_t pack_joint(int mode, int column) { return (int32_t)((uint32_t)mode | ((uint32_t)(column + 1) << 2)); }
JXS_ENV_HD int packed_mode(int32_t code) { return code & 3; }
JXS_ENV_HD int packed_column(int32_t code) { return (int)((uint32_t)code >> 2) - 1; }
template <typename T>
struct alignas(16) Params {
  T v[kParams];
};

}  // namespace jxs_act

#if !defined(__clang__)
#pragma GCC pop_options
#endif
