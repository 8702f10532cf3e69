// The contact sensors of one environment as plain functions (jxs_env_contacts in jxs_api.hip): from the tiled link transforms
// [nL*12][N] and inertial-fixed link velocities [nL*6][N] of jxs_refresh_kinematics to a tiled record [G*kRows][N] of foot
// contact, clearance, slip and air time per group of points, laid out as a source block of jxs_env_observe and
// jxs_env_evaluate.  Plain functions for host and device, no HIP types.  sense_env() is everything of one environment;
// tests/emul/jxs_emul_env_contact.cpp drives it over every environment on the CPU.  The kernel evaluates the same pieces:
// point_sample() once per (point, environment), fold() per point of a group in entry order, finish() per group.
//
// A sensor table has P entries (1 <= P <= kMaxPoints), entry k = {parent link, L_p[3]}, in G groups (1 <= G <= kMaxGroups)
// {first, count >= 1} whose ranges are disjoint and cover every entry.  Per environment and entry, with [R|t] the twelve
// transform rows (row-major, 12 link + 4 r + c) and (v, w) the six velocity rows (6 link + 0..2 linear, 3..5 angular) of its
// parent link:
//   p_i  = ((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i]                 (api/contact.py:18-45, rbda/collidable_points.py:9-65)
//   pd   = v + w x p,  (w x p)_0 = w_1 p_2 - w_2 p_1, ...               (the same lines; jxs_rand::cross_component)
//   h    = height(p_x, p_y), the operations of the step kernel (jxs_core.h hf_height, terrain_normal_and_depth):
//            flat         terrain_h
//            plane        terrain_h - (n_x p_x + n_y p_y) * (1 / n_z)
//            height field fx = fmin(fmax((x - x0) * idx, 0), nx - 1), ix = (int)fmin(fx, nx - 2), tx = fx - ix, alike in y;
//                         a = h00 + (h01 - h00) ty, c = h10 + (h11 - h10) ty, h = a + (c - a) tx of hf[ix * ny + iy + ...]
//                         (fmin and fmax drop a NaN: a NaN coordinate reads the first border sample)
//   c    = p_z - h;  the point is in contact when c <= 0 (src/jaxsim/api/contact.py:92-145); a NaN c is no contact
//   s    = |pd - (pd . n) n|^2 = (t_0 t_0 + t_1 t_1) + t_2 t_2, t_i = pd_i - d n_i, d = (pd_0 n_0 + pd_1 n_1) + pd_2 n_2, with n the
//          terrain normal: flat +z, where s = pd_x pd_x + pd_y pd_y; plane the constant normal; height field (gx, gy, 1) r with
//          g = (h(x - delta) - h(x + delta)) * inv_2delta and r = 1 / sqrt((gx gx + gy gy) + 1), the one place with a square
//          root and a division.  Without a velocity block s = 0.
// Per group, in entry order: count of points in contact; m = c_first, then m = c_k < m ? c_k : m; the largest s over the
// points in contact (a NaN s is passed over), 0 without one.  Then with the timers (a, b) of the group, zeroed first where the
// reset mask says so:  touchdown = contact && a > 0;  a' = contact ? 0 : a + dt;  b' = contact ? b + dt : 0;  rows kFlag ..
// kFlightTime of the record are {contact, count, m, slip, a', b', touchdown, touchdown ? a : 0}.  Without timers rows 4-7 are 0.
//
// Arithmetic is done in the block's type and every operation is rounded on its own (jxs_env_random.h: contraction off for
// hipcc and g++), so that host and device give the same bits except for the slip on a height field.
#pragma once

#include <cmath>
#include <cstdint>

#include "jxs_env_observe.h"
#include "jxs_env_ops.h"
#include "jxs_env_random.h"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace jxs_contact {

// JXS_CONTACT_* of include/jaxsim_amd.h
constexpr int kMaxPoints = 1024, kMaxGroups = 32;
constexpr int kRows = 8, kTimerRows = 2;
constexpr int kFlag = 0, kCount = 1, kClearance = 2, kSlipSq = 3, kAirTime = 4, kContactTime = 5, kTouchdown = 6, kFlightTime = 7;
constexpr int kTerrainFlat = 0, kTerrainPlane = 1, kTerrainField = 2;

// the terrain of a model (KParams of jxs_params.h) with its height-field samples
template <typename T>
struct Terrain {
  int kind;            // kTerrain*
  T height;            // terrain_h
  T normal[3];         // the plane's unit normal
  T inv_nz;            // 1 / normal[2], rounded once
  int nx, ny;          // samples per axis
  T x0, y0, idx, idy;  // origin, 1 / spacing
  T delta, inv_2delta;
  const T* samples;  // [nx][ny]
};

JXS_ENV_HD float lesser(float a, float b) { return fminf(a, b); }
JXS_ENV_HD double lesser(double a, double b) { return fmin(a, b); }
JXS_ENV_HD float greater(float a, float b) { return fmaxf(a, b); }
JXS_ENV_HD double greater(double a, double b) { return fmax(a, b); }

// the bilinear interpolant of the samples, clamped to the border samples outside the grid
template <typename T>
JXS_ENV_HD T field_height(const Terrain<T>& tr, T x, T y) {
  JXS_RAND_NO_CONTRACT
  const T fx = lesser(greater((x - tr.x0) * tr.idx, T(0)), T(tr.nx - 1));
  const T fy = lesser(greater((y - tr.y0) * tr.idy, T(0)), T(tr.ny - 1));
  const int ix = (int)lesser(fx, T(tr.nx - 2)), iy = (int)lesser(fy, T(tr.ny - 2));
  const T tx = fx - T(ix), ty = fy - T(iy);
  const int b = ix * tr.ny + iy;
  const T h00 = tr.samples[b], h01 = tr.samples[b + 1], h10 = tr.samples[b + tr.ny], h11 = tr.samples[b + tr.ny + 1];
  const T a = h00 + (h01 - h00) * ty, c = h10 + (h11 - h10) * ty;
  return a + (c - a) * tx;
}

template <typename T>
JXS_ENV_HD T terrain_height(const Terrain<T>& tr, T x, T y) {
  JXS_RAND_NO_CONTRACT
  if (tr.kind == kTerrainField) return field_height(tr, x, y);
  if (tr.kind == kTerrainPlane) return tr.height - (tr.normal[0] * x + tr.normal[1] * y) * tr.inv_nz;
  return tr.height;
}

// the unit normal at (x, y) where the terrain is not flat
template <typename T>
JXS_ENV_HD void terrain_normal(const Terrain<T>& tr, T x, T y, T n[3]) {
  JXS_RAND_NO_CONTRACT
  if (tr.kind != kTerrainField) {
    n[0] = tr.normal[0], n[1] = tr.normal[1], n[2] = tr.normal[2];
    return;
  }
  const T hxp = field_height(tr, x + tr.delta, y), hxm = field_height(tr, x - tr.delta, y);
  const T hyp = field_height(tr, x, y + tr.delta), hym = field_height(tr, x, y - tr.delta);
  const T gx = (hxm - hxp) * tr.inv_2delta, gy = (hym - hyp) * tr.inv_2delta;
  const T r = T(1) / jxs_obs::square_root((gx * gx + gy * gy) + T(1));
  n[0] = gx * r, n[1] = gy * r, n[2] = r;
}

// squared norm of the part of pd tangential to the terrain at (x, y)
template <typename T>
JXS_ENV_HD T slip_squared(const Terrain<T>& tr, T x, T y, const T pd[3]) {
  JXS_RAND_NO_CONTRACT
  if (tr.kind == kTerrainFlat) return pd[0] * pd[0] + pd[1] * pd[1];
  T n[3];
  terrain_normal(tr, x, y, n);
  const T d = (pd[0] * n[0] + pd[1] * n[1]) + pd[2] * n[2];
  const T t0 = pd[0] - d * n[0], t1 = pd[1] - d * n[1], t2 = pd[2] - d * n[2];
  return (t0 * t0 + t1 * t1) + t2 * t2;
}

template <typename T>
struct Sample {
  T clearance, slip_sq;
};

// One point of one environment: link(r) is row r (0 .. 11) of the transform of its parent link, vel(r) row r (0 .. 5) of its
// velocity; the velocity is read only for a point in contact (no other point's slip reaches the record)
template <typename T, typename Link, typename Vel>
JXS_ENV_HD Sample<T> point_sample(const Terrain<T>& tr, const T L_p[3], bool has_velocity, Link link, Vel vel) {
  JXS_RAND_NO_CONTRACT
  T p[3];
  for (int i = 0; i < 3; ++i) p[i] = ((link(4 * i) * L_p[0] + link(4 * i + 1) * L_p[1]) + link(4 * i + 2) * L_p[2]) + link(4 * i + 3);
  Sample<T> s{p[2] - terrain_height(tr, p[0], p[1]), T(0)};
  if (has_velocity && s.clearance <= T(0)) {
    const T w[3] = {vel(3), vel(4), vel(5)};
    T pd[3];
    for (int i = 0; i < 3; ++i) pd[i] = vel(i) + jxs_rand::cross_component(w, p, i);
    s.slip_sq = slip_squared(tr, p[0], p[1], pd);
  }
  return s;
}

// what a group has seen of its points so far
template <typename T>
struct Fold {
  T count, clearance, slip_sq;
};
template <typename T>
JXS_ENV_HD Fold<T> fold(bool first, Fold<T> f, const Sample<T>& s) {
  JXS_RAND_NO_CONTRACT
  if (first) f = Fold<T>{T(0), s.clearance, T(0)};
  else f.clearance = s.clearance < f.clearance ? s.clearance : f.clearance;
  if (s.clearance <= T(0)) {
    f.count = f.count + T(1);
    f.slip_sq = s.slip_sq > f.slip_sq ? s.slip_sq : f.slip_sq;
  }
  return f;
}

// the record rows of a group and its new timers (a, b); `timed` false: no timer block, rows 4-7 are zero
template <typename T>
JXS_ENV_HD void finish(const Fold<T>& f, bool timed, bool reset, T dt, T* a, T* b, T rec[kRows]) {
  JXS_RAND_NO_CONTRACT
  const bool contact = f.count > T(0);
  rec[kFlag] = contact ? T(1) : T(0), rec[kCount] = f.count, rec[kClearance] = f.clearance, rec[kSlipSq] = f.slip_sq;
  for (int r = kAirTime; r < kRows; ++r) rec[r] = T(0);
  if (!timed) return;
  const T a0 = reset ? T(0) : *a, b0 = reset ? T(0) : *b;
  const bool touchdown = contact && a0 > T(0);
  *a = contact ? T(0) : a0 + dt;
  *b = contact ? b0 + dt : T(0);
  rec[kAirTime] = *a, rec[kContactTime] = *b, rec[kTouchdown] = touchdown ? T(1) : T(0), rec[kFlightTime] = touchdown ? a0 : T(0);
}

// A table as the host holds it
template <typename T>
struct Table {
  int G, P;
  const int32_t* groups;  // [G][2] {first, count}
  const int32_t* parent;  // [P]
  const T* L_p;           // [P][3]
};

// Everything of one environment: link(l, r) and vel(l, r) are the rows of link l, timer(r) the environment's timer row r
// (in/out, a of group g at 2g, b at 2g + 1; read and written only when `timed`), record(r, x) takes row r of its record
template <typename T, typename Link, typename Vel, typename Timer, typename Record>
JXS_ENV_HD void sense_env(const Terrain<T>& tr, const Table<T>& tb, bool has_velocity, bool timed, bool reset, T dt, Link link, Vel vel, Timer timer,
                          Record record) {
  for (int g = 0; g < tb.G; ++g) {
    const int first = tb.groups[2 * g], count = tb.groups[2 * g + 1];
    Fold<T> f{T(0), T(0), T(0)};
    for (int k = first; k < first + count; ++k) {
      const int l = tb.parent[k];
      f = fold(k == first, f, point_sample(tr, tb.L_p + 3 * k, has_velocity, [&](int r) { return link(l, r); }, [&](int r) { return vel(l, r); }));
    }
    T a = T(0), b = T(0), rec[kRows];
    if (timed) a = *timer(kTimerRows * g), b = *timer(kTimerRows * g + 1);
    finish(f, timed, reset, dt, &a, &b, rec);
    if (timed) *timer(kTimerRows * g) = a, *timer(kTimerRows * g + 1) = b;
    for (int r = 0; r < kRows; ++r) record(kRows * g + r, rec[r]);
  }
}

// Validity of a table in double precision as the create call receives it.  kOk, or the first error and the group or entry
// it is in (-1: the table as a whole).  Groups are checked first, in order, then the entries.
constexpr int kOk = 0, kBadSize = 1, kBadGroup = 2, kUncovered = 3, kBadParent = 4, kNotFinite = 5;
JXS_ENV_HD int table_error(long long G, const int32_t* groups, long long P, const int32_t* parent, const double* L_p, int n_links, bool single,
                           int* bad) {
  *bad = -1;
  if (G < 1 || G > kMaxGroups || P < 1 || P > kMaxPoints || groups == nullptr || parent == nullptr || L_p == nullptr) return kBadSize;
  bool owned[kMaxPoints] = {};
  for (int g = 0; g < (int)G; ++g) {
    const int first = groups[2 * g], count = groups[2 * g + 1];
    *bad = g;
    if (count < 1 || first < 0 || (long long)first + count > P) return kBadGroup;  // (empty, or outside the table)
    for (int k = first; k < first + count; ++k) {
      if (owned[k]) return kBadGroup;  // (overlaps an earlier group)
      owned[k] = true;
    }
  }
  for (int k = 0; k < (int)P; ++k) {
    *bad = k;
    if (!owned[k]) return kUncovered;
    if (parent[k] < 0 || parent[k] >= n_links) return kBadParent;
    for (int i = 0; i < 3; ++i)
      if (!(single ? jxs_obs::affine_ok(L_p[3 * k + i], 0.0f) : jxs_obs::affine_ok(L_p[3 * k + i], 0.0))) return kNotFinite;
  }
  *bad = -1;
  return kOk;
}

}  // namespace jxs_contact

#if !defined(__clang__)
#pragma GCC pop_options
#endif
