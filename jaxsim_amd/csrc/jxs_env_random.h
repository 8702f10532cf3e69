// The random reset state of one environment as plain functions (jxs_env_randomize in jxs_api.hip): the Philox4x32-10
// block function, the uniform variables drawn from it, and the word of the state block that each row takes from them.
// Plain functions for host and device, no HIP types.  row_value() is the word of a row of an environment;
// tests/emul/jxs_emul_env_random.cpp drives it over every word on the CPU.  The kernel evaluates the same three pieces
// row_value() is made of, each once per environment instead of once per word: variable() for every variable, derived_value()
// on those for the ten rows that are no variable (quaternion, converted base velocity), row_source() to place them.
//
// What a value depends on: (seed, draw, global environment index, variable index) and the bounds table -- never on
// N, the tiling, the mask or how a batch is split over processes.
//   key     = (seed low, seed high)
//   counter = (global environment, variable, draw low, draw high)
// One Philox block per variable; its words 0 and 1 make the uniform, words 2 and 3 are unused.
//
// Variables of a model with n joints, 12 + 2n of them (`bounds` is [2][12 + 2n]: the row of lower, the row of upper bounds):
//   0-2 base position | 3-5 XYZ Euler angles | 6 .. 5+n joint positions |
//   6+n .. 8+n base linear velocity | 9+n .. 11+n base angular velocity | 12+n .. 11+2n joint velocities
//
// Rows of the state block (jaxsim_amd/state.py): position = variables 0-2; quaternion wxyz of R = Rx(a0) Ry(a1) Rz(a2)
// (the reference's Rotation.from_euler("XYZ"), src/jaxsim/api/data.py:624-631); joint positions; the base velocity,
// sampled as (l, a) in the caller's representation and stored inertial-fixed [l' + p x a' ; a'] with (l', a') = (l, a)
// for Mixed, (R l, R a) for Body -- Inertial stores the sampled (l, a) themselves --, six exact zeros for a fixed base;
// joint velocities; every row behind them (tangential deformation) is zero, the reference's default contact state.
//
// Arithmetic is done in the block's type and every operation is rounded on its own: the functions below switch the
// contraction of a multiply and an add into one fused operation off, for hipcc (clang) and for g++, so that host and
// device give the same bits wherever no sine or cosine is involved.
#pragma once

#include <cmath>
#include <cstdint>

#include "jxs_env_ops.h"

#if defined(__clang__)
#define JXS_RAND_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JXS_RAND_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace jxs_rand {

constexpr int kReprInertial = 0, kReprBody = 1, kReprMixed = 2;  // JXS_REPR_* of include/jaxsim_amd.h

JXS_ENV_HD int n_variables(int n_joints) { return 12 + 2 * n_joints; }

// first_env + e must fit the 32 bits of counter word 0 for every e < N
JXS_ENV_HD bool env_range_ok(long long first_env, long long N) { return first_env >= 0 && first_env + N <= (1LL << 32); }

JXS_ENV_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b >> 32); }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
JXS_ENV_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// words 0 and 1 of the block of variable v of a global environment
JXS_ENV_HD void draw_words(uint64_t seed, uint64_t draw, uint32_t env_global, int v, uint32_t* w0, uint32_t* w1) {
  const uint32_t ctr[4] = {env_global, (uint32_t)v, (uint32_t)draw, (uint32_t)(draw >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t out[4];
  philox4x32_10(ctr, key, out);
  *w0 = out[0], *w1 = out[1];
}

// u in [0, 1): 24 bits in float, 53 bits in double, both exact
JXS_ENV_HD float unit_uniform(uint32_t w0, uint32_t, float) { return (float)(w0 >> 8) * 5.9604644775390625e-8f; }
JXS_ENV_HD double unit_uniform(uint32_t w0, uint32_t w1, double) {
  return (double)(((uint64_t)(w0 >> 5) << 26) + (uint64_t)(w1 >> 6)) * 1.1102230246251565404e-16;
}

// x = lo + u (hi - lo), three roundings, clamped from above; lo == hi gives lo
template <typename T>
JXS_ENV_HD T scale_uniform(T u, T lo, T hi) {
  JXS_RAND_NO_CONTRACT
  const T d = hi - lo;
  const T m = u * d;
  const T x = lo + m;
  return x > hi ? hi : x;
}

// variable v of a global environment
template <typename T>
JXS_ENV_HD T variable(const T* bounds, int nv, int v, uint64_t seed, uint64_t draw, uint32_t env_global) {
  uint32_t w0, w1;
  draw_words(seed, draw, env_global, v, &w0, &w1);
  return scale_uniform(unit_uniform(w0, w1, T(0)), bounds[v], bounds[nv + v]);
}

JXS_ENV_HD void sin_cos(float x, float* s, float* c) { *s = sinf(x), *c = cosf(x); }
JXS_ENV_HD void sin_cos(double x, double* s, double* c) { *s = sin(x), *c = cos(x); }

// wxyz quaternion of Rx(a0) Ry(a1) Rz(a2) = qx qy qz; products left to right
template <typename T>
JXS_ENV_HD void euler_xyz_to_quaternion(const T a[3], T q[4]) {
  JXS_RAND_NO_CONTRACT
  T sx, cx, sy, cy, sz, cz;
  sin_cos(a[0] * T(0.5), &sx, &cx);
  sin_cos(a[1] * T(0.5), &sy, &cy);
  sin_cos(a[2] * T(0.5), &sz, &cz);
  const T ccc = cx * cy * cz, sss = sx * sy * sz, scc = sx * cy * cz, css = cx * sy * sz;
  const T csc = cx * sy * cz, scs = sx * cy * sz, ccs = cx * cy * sz, ssc = sx * sy * cz;
  q[0] = ccc - sss, q[1] = scc + css, q[2] = csc - scs, q[3] = ccs + ssc;
}

// row k of the rotation matrix of a unit quaternion wxyz, times x
template <typename T>
JXS_ENV_HD T rotate_component(const T q[4], const T x[3], int k) {
  JXS_RAND_NO_CONTRACT
  const T w = q[0], i = q[1], j = q[2], l = q[3];
  T r0, r1, r2;
  if (k == 0) r0 = T(1) - T(2) * (j * j + l * l), r1 = T(2) * (i * j - w * l), r2 = T(2) * (i * l + w * j);
  else if (k == 1) r0 = T(2) * (i * j + w * l), r1 = T(1) - T(2) * (i * i + l * l), r2 = T(2) * (j * l - w * i);
  else r0 = T(2) * (i * l - w * j), r1 = T(2) * (j * l + w * i), r2 = T(1) - T(2) * (i * i + j * j);
  return r0 * x[0] + r1 * x[1] + r2 * x[2];
}

// component k of p x a
template <typename T>
JXS_ENV_HD T cross_component(const T p[3], const T a[3], int k) {
  JXS_RAND_NO_CONTRACT
  const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
  return p[k1] * a[k2] - p[k2] * a[k1];
}

struct Shape {
  int n_joints;  // the rows are those of jaxsim_amd/state.py: 13 + 2n sampled ones, zero rows behind them
  int floating;  // 0: the six base-velocity rows are zero
  int repr;      // representation the base velocity is sampled in (kRepr*)
};

// Where the word of a row comes from: a variable as it is, one of the kDerived values computed from several variables
// (0-3 the quaternion wxyz, 4-6 the stored linear, 7-9 the stored angular base velocity), or zero
constexpr int kRowZero = 0, kRowVariable = 1, kRowDerived = 2;
constexpr int kDerived = 10;
struct RowSource {
  int kind;   // kRow*
  int index;  // variable or derived value
};

JXS_ENV_HD RowSource row_source(const Shape& sh, int row) {
  const int n = sh.n_joints, row_vlin = 7 + n, row_sd = 13 + n;
  if (row < 3) return RowSource{kRowVariable, row};
  if (row < 7) return RowSource{kRowDerived, row - 3};
  if (row < row_vlin) return RowSource{kRowVariable, row - 1};
  if (row < row_sd) {
    const int c = row - row_vlin;  // 0-2 linear, 3-5 angular
    if (!sh.floating) return RowSource{kRowZero, 0};
    if (sh.repr == kReprInertial || (sh.repr == kReprMixed && c >= 3)) return RowSource{kRowVariable, 6 + n + c};
    return RowSource{kRowDerived, 4 + c};
  }
  if (row < row_sd + n) return RowSource{kRowVariable, row - 1};
  return RowSource{kRowZero, 0};
}

// Derived value d of an environment whose variable v is var(v).  Only the values row_source() names are defined:
// the velocity ones for a floating base in Mixed (linear) and Body (all six) representation.
template <typename T, typename Var>
JXS_ENV_HD T derived_value(const Shape& sh, int d, Var var) {
  JXS_RAND_NO_CONTRACT
  const int n = sh.n_joints, v_lin = 6 + n, v_ang = 9 + n;
  T a[3], q[4];
  if (d < 4 || sh.repr == kReprBody) {
    for (int k = 0; k < 3; ++k) a[k] = var(3 + k);
    euler_xyz_to_quaternion(a, q);
    if (d < 4) return q[d];
  }
  const int k = (d - 4) % 3;
  const bool linear = d < 7;
  T ang[3];
  for (int c = 0; c < 3; ++c) ang[c] = var(v_ang + c);
  if (sh.repr == kReprBody) {
    if (!linear) return rotate_component(q, ang, k);
    const T rotated[3] = {rotate_component(q, ang, 0), rotate_component(q, ang, 1), rotate_component(q, ang, 2)};
    for (int c = 0; c < 3; ++c) ang[c] = rotated[c];
  }
  T p[3];
  for (int c = 0; c < 3; ++c) p[c] = var(c);
  T lin_k;
  if (sh.repr == kReprBody) {
    T lin[3];
    for (int c = 0; c < 3; ++c) lin[c] = var(v_lin + c);
    lin_k = rotate_component(q, lin, k);
  } else {
    lin_k = var(v_lin + k);
  }
  return lin_k + cross_component(p, ang, k);
}

// The word of `row` of the state of a global environment
template <typename T>
JXS_ENV_HD T row_value(const Shape& sh, int row, const T* bounds, uint64_t seed, uint64_t draw, uint32_t env_global) {
  const int nv = n_variables(sh.n_joints);
  const RowSource src = row_source(sh, row);
  auto var = [&](int v) { return variable(bounds, nv, v, seed, draw, env_global); };
  if (src.kind == kRowVariable) return var(src.index);
  if (src.kind == kRowDerived) return derived_value<T>(sh, src.index, var);
  return T(0);
}

}  // namespace jxs_rand

#if !defined(__clang__)
#pragma GCC pop_options
#endif
