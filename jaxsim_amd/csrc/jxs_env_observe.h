// A policy observation of one environment as plain functions (jxs_env_observe in jxs_api.hip): the environment-major
// tensor [N][D] a network reads, assembled from the tiled state block and up to four further tiled blocks.  Plain
// functions for host and device, no HIP types.  slot_value() is one word of the tensor;
// tests/emul/jxs_emul_env_observe.cpp drives it over every word on the CPU.  The kernel evaluates the same pieces
// slot_value() is made of, each once per environment instead of once per word: unit_quaternion_component() for the four
// words of q / |q|, derived_from_unit() on those for the other 18 derived values, slot_raw() / affine() to place them.
//
// An observation is D slots (1 <= D <= kMaxWidth), slot d = {kind, source, index} with an offset[d] and a scale[d] in
// the block's type.  Word d of environment e is (x - offset[d]) * scale[d], two roundings, never fused; x by kind:
//   kStateRow          word `index` of the environment's state rows (jaxsim_amd/state.py order)
//   kSourceRow         row `index` of auxiliary block `source` (0 .. 3): a tiled [rows_s][N] array of the state's type and tile
//   kBaseQuatUnit      component `index` (w x y z) of q^ = q / |q|; |q| = 0 leaves q as it is (the rule of the host's
//                      data.base_orientation; the reference's src/jaxsim/api/data.py:267-286)
//   kBaseRotation      entry `index` (0 .. 8, row-major) of R(q^)
//   kBaseVelocity      component `index` (0-2 linear, 3-5 angular) of the base velocity in the launch's representation: the
//                      inverse of the storage rule at the top of jxs_env_random.h (the reference's
//                      src/jaxsim/api/data.py:288-312, inertial_to_other_representation of api/common.py:100-158).  With the
//                      stored (l, w) and the base position p: Inertial (l, w); Mixed (l - p x w, w);
//                      Body (R^T (l - p x w), R^T w).  The stored rows of a fixed base are treated alike.
//   kProjectedGravity  component `index` of R^T (0, 0, -1)
//
// Arithmetic is done in the block's type and every operation is rounded on its own (jxs_env_random.h: contraction off for
// hipcc and g++), so that host and device give the same bits wherever no square root or division is involved: the state
// and source rows, the Inertial and the Mixed velocity.
#pragma once

#include <cmath>
#include <cstdint>

#include "jxs_env_ops.h"
#include "jxs_env_random.h"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace jxs_obs {

constexpr int kMaxWidth = 4096;  // JXS_OBS_MAX_WIDTH of include/jaxsim_amd.h
constexpr int kSources = 4;
// JXS_OBS_* of include/jaxsim_amd.h
constexpr int kStateRow = 0, kSourceRow = 1, kBaseQuatUnit = 2, kBaseRotation = 3, kBaseVelocity = 4, kProjectedGravity = 5;
constexpr int kKinds = 6;
// The derived values of an environment: 0-3 q^ (w x y z), 4-12 R(q^) row-major, 13-18 the base velocity, 19-21 the
// projected gravity
constexpr int kDerived = 22;
constexpr int kDerivedQuat = 0, kDerivedRot = 4, kDerivedVel = 13, kDerivedGrav = 19;

struct Slot {
  int32_t kind, source, index;
};

struct Shape {
  int n_rows;    // rows of the state block (jaxsim_amd/state.py)
  int n_joints;  // position 0-2, quaternion 3-6, linear velocity 7+n .. 9+n, angular velocity 10+n .. 12+n
  int repr;      // representation of kBaseVelocity (jxs_rand::kRepr*)
};

JXS_ENV_HD int row_pos(const Shape&) { return 0; }
JXS_ENV_HD int row_quat(const Shape&) { return 3; }
JXS_ENV_HD int row_vlin(const Shape& sh) { return 7 + sh.n_joints; }
JXS_ENV_HD int row_vang(const Shape& sh) { return 10 + sh.n_joints; }

// components of a slot of each kind (state and source rows are bounded by their block instead)
JXS_ENV_HD int kind_components(int kind) {
  return kind == kBaseQuatUnit ? 4 : kind == kBaseRotation ? 9 : kind == kBaseVelocity ? 6 : kind == kProjectedGravity ? 3 : 0;
}

// derived value a slot of a derived kind reads
JXS_ENV_HD int derived_index(int kind, int index) {
  return (kind == kBaseQuatUnit ? kDerivedQuat : kind == kBaseRotation ? kDerivedRot : kind == kBaseVelocity ? kDerivedVel : kDerivedGrav) + index;
}

// Validity of a slot table against the rows of the state and of the four sources (rows_s[s] <= 0: no such source)
constexpr int kOk = 0, kBadWidth = 1, kBadKind = 2, kBadIndex = 3, kBadSource = 4;
JXS_ENV_HD int slot_error(const Slot& s, int n_rows, const int32_t* rows_s) {
  if (s.kind < 0 || s.kind >= kKinds) return kBadKind;
  if (s.kind == kStateRow) return s.index >= 0 && s.index < n_rows ? kOk : kBadIndex;
  if (s.kind == kSourceRow) {
    if (s.source < 0 || s.source >= kSources || rows_s == nullptr || rows_s[s.source] <= 0) return kBadSource;
    return s.index >= 0 && s.index < rows_s[s.source] ? kOk : kBadIndex;
  }
  return s.index >= 0 && s.index < kind_components(s.kind) ? kOk : kBadIndex;
}
// kOk, or the first error and the slot it is in; `slots` is [D][3]
JXS_ENV_HD int table_error(const int32_t* slots, long long D, int n_rows, const int32_t* rows_s, int* bad_slot) {
  *bad_slot = -1;
  if (D < 1 || D > kMaxWidth || slots == nullptr) return kBadWidth;
  for (int d = 0; d < (int)D; ++d) {
    const int e = slot_error(Slot{slots[3 * d], slots[3 * d + 1], slots[3 * d + 2]}, n_rows, rows_s);
    if (e != kOk) {
      *bad_slot = d;
      return e;
    }
  }
  return kOk;
}

// an offset or a scale must be finite in the block's type
JXS_ENV_HD bool affine_ok(double v, float) { return v - v == 0.0 && (float)v - (float)v == 0.0f; }
JXS_ENV_HD bool affine_ok(double v, double) { return v - v == 0.0; }

// Which derived values a table needs, as bits: those its slots read, and q^ for every value computed from it
JXS_ENV_HD uint32_t derived_needing_quat(int repr) {
  uint32_t m = (0x1ffu << kDerivedRot) | (0x7u << kDerivedGrav);
  if (repr == jxs_rand::kReprBody) m |= 0x3fu << kDerivedVel;
  return m;
}
JXS_ENV_HD uint32_t derived_used(const int32_t* slots, int D, int repr) {
  uint32_t used = 0;
  for (int d = 0; d < D; ++d)
    if (slots[3 * d] >= kBaseQuatUnit) used |= 1u << derived_index(slots[3 * d], slots[3 * d + 2]);
  if (used & derived_needing_quat(repr)) used |= 0xfu << kDerivedQuat;
  return used;
}

// the word of a slot: one rounding for the difference, one for the product
template <typename T>
JXS_ENV_HD T affine(T x, T offset, T scale) {
  JXS_RAND_NO_CONTRACT
  const T d = x - offset;
  return d * scale;
}

JXS_ENV_HD float square_root(float x) { return sqrtf(x); }
JXS_ENV_HD double square_root(double x) { return sqrt(x); }

// component k of q / |q|, the squares summed left to right; |q| = 0 leaves q as it is
template <typename T>
JXS_ENV_HD T unit_quaternion_component(const T q[4], int k) {
  JXS_RAND_NO_CONTRACT
  const T n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const T nrm = square_root(n2);
  return nrm == T(0) ? q[k] : q[k] / nrm;
}

// Derived value d >= kDerivedRot of an environment whose unit quaternion is u and whose state row r is row(r).
// R^T x is the rotation by the conjugate of u.
template <typename T, typename Row>
JXS_ENV_HD T derived_from_unit(const Shape& sh, int d, const T u[4], Row row) {
  JXS_RAND_NO_CONTRACT
  if (d < kDerivedVel) {  // entry (r, c) of R: row r of R times the unit vector c
    const int r = (d - kDerivedRot) / 3, c = (d - kDerivedRot) % 3;
    const T unit[3] = {c == 0 ? T(1) : T(0), c == 1 ? T(1) : T(0), c == 2 ? T(1) : T(0)};
    return jxs_rand::rotate_component(u, unit, r);
  }
  const T conj[4] = {u[0], -u[1], -u[2], -u[3]};
  if (d >= kDerivedGrav) {
    const T down[3] = {T(0), T(0), T(-1)};
    return jxs_rand::rotate_component(conj, down, d - kDerivedGrav);
  }
  const int c = d - kDerivedVel, k = c % 3;
  const bool linear = c < 3;
  if (sh.repr == jxs_rand::kReprInertial || (sh.repr == jxs_rand::kReprMixed && !linear)) return row((linear ? row_vlin(sh) : row_vang(sh)) + k);
  T ang[3];
  for (int i = 0; i < 3; ++i) ang[i] = row(row_vang(sh) + i);
  if (!linear) return jxs_rand::rotate_component(conj, ang, k);  // (Body)
  T p[3];
  for (int i = 0; i < 3; ++i) p[i] = row(row_pos(sh) + i);
  if (sh.repr == jxs_rand::kReprMixed) return row(row_vlin(sh) + k) - jxs_rand::cross_component(p, ang, k);
  T m[3];
  for (int i = 0; i < 3; ++i) m[i] = row(row_vlin(sh) + i) - jxs_rand::cross_component(p, ang, i);
  return jxs_rand::rotate_component(conj, m, k);
}

// Derived value d (0 .. kDerived-1) of an environment from its state rows alone
template <typename T, typename Row>
JXS_ENV_HD T derived_value(const Shape& sh, int d, Row row) {
  T q[4] = {T(0), T(0), T(0), T(0)}, u[4] = {T(0), T(0), T(0), T(0)};
  if (d < kDerivedRot || ((derived_needing_quat(sh.repr) >> d) & 1u)) {
    for (int k = 0; k < 4; ++k) q[k] = row(row_quat(sh) + k);
    if (d < kDerivedRot) return unit_quaternion_component(q, d);
    for (int k = 0; k < 4; ++k) u[k] = unit_quaternion_component(q, k);
  }
  return derived_from_unit<T>(sh, d, u, row);
}

// x of a slot: row(r) is word r of the environment's state rows, src(s, r) row r of its source s
template <typename T, typename Row, typename Src>
JXS_ENV_HD T slot_raw(const Shape& sh, const Slot& s, Row row, Src src) {
  if (s.kind == kStateRow) return row(s.index);
  if (s.kind == kSourceRow) return src(s.source, s.index);
  return derived_value<T>(sh, derived_index(s.kind, s.index), row);
}

// The word of slot `s` of an environment
template <typename T, typename Row, typename Src>
JXS_ENV_HD T slot_value(const Shape& sh, const Slot& s, T offset, T scale, Row row, Src src) {
  return affine(slot_raw<T>(sh, s, row, src), offset, scale);
}

// The table as the kernel reads it: one word per slot, kind | source << 3 | index << 5.  A derived kind is stored with
// its derived value as index.
JXS_ENV_HD int32_t pack_slot(const Slot& s) {
  const int index = s.kind >= kBaseQuatUnit ? derived_index(s.kind, s.index) : s.index;
  return (int32_t)((uint32_t)s.kind | ((uint32_t)(s.kind == kSourceRow ? s.source : 0) << 3) | ((uint32_t)index << 5));
}
JXS_ENV_HD int packed_kind(int32_t code) { return code & 7; }
JXS_ENV_HD int packed_source(int32_t code) { return (code >> 3) & 3; }
JXS_ENV_HD int packed_index(int32_t code) { return (int)((uint32_t)code >> 5); }

}  // namespace jxs_obs

#if !defined(__clang__)
#pragma GCC pop_options
#endif
