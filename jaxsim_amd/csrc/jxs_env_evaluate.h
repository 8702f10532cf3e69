// The reward and the termination flags of one environment as plain functions (jxs_env_evaluate in jxs_api.hip): one word
// `reward`, one byte `done` (bit 0 terminated, bit 1 truncated: the mask of jxs_env_select and jxs_env_randomize as it is),
// optionally a word `fired` of the conditions that fired, the per-term contributions and an episode counter.  Plain
// functions for host and device, no HIP types.  evaluate_env() is everything of one environment;
// tests/emul/jxs_emul_env_evaluate.cpp drives it over every environment on the CPU.  The kernel evaluates the same pieces:
// slot_x() / jxs_obs::affine() for a slot, term_value() for a term, fires() for a condition, total() and counted() for the
// rest.
//
// A table holds D slots (1 <= D <= kMaxSlots) that read what an observation slot reads (jxs_env_observe.h: state rows, the
// four sources, the derived kinds), each with an offset and a scale, and each optionally with a target {source, row}
// (source -1: none), the per-environment commanded value:
//   x_d = target ? raw_d - src(source, row) : raw_d                    (one rounding)
//   y_d = (x_d - offset_d) * scale_d                                   (jxs_obs::affine)
// Every slot belongs to exactly one term or one condition.
//
// Term t (0 <= K <= kMaxTerms) = {first, count >= 1, inner, outer} with {weight, lo, hi} owns slots first .. first+count-1:
//   v_d = inner(y_d):  kIdentity y | kAbs |y| | kSquare y * y | kExcess d = |y| - 1, d < 0 ? 0 : d  (max(|y| - 1, 0); a NaN stays)
//   s   = v_first, then s = s + v_d in slot order                      (strictly sequential)
//   o   = outer(s):    kOuterIdentity s | kOuterExp exp(-s)            (the accurate exponential of the block's type)
//   p_t = clamp(weight * o, lo, hi)                                    (jxs_act::clamp: comparisons, a NaN stays a NaN)
// and r = p_0, then r = r + p_t in term order; r = clamp(r, reward_lo, reward_hi); K = 0 starts from r = 0.
//
// Condition c (0 <= C <= kMaxConditions) = {slot, kind} with {lo, hi} fires when !(lo <= y && y <= hi) -- so a NaN fires --,
// sets the bit of its kind (kTerminated, kTruncated) in `done` and bit c in `fired`.
//
// The counter (optional, max_steps > 0): n = steps + 1; n >= max_steps sets kTruncated (no bit of `fired`); then
// steps = done ? 0 : n.  Last, a terminated environment (bit 0 of done) has termination_reward added to r.
//
// Arithmetic is done in the block's type and every operation is rounded on its own (jxs_env_random.h: contraction off for
// hipcc and g++).  Apart from what a derived slot reads (jxs_env_observe.h) only the exponential differs between host and
// device, by the error of the two implementations.
#pragma once

#include <cmath>
#include <cstdint>

#include "jxs_env_act.h"
#include "jxs_env_observe.h"
#include "jxs_env_ops.h"
#include "jxs_env_random.h"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace jxs_eval {

// JXS_EVAL_MAX_* of include/jaxsim_amd.h
constexpr int kMaxSlots = 1024, kMaxTerms = 32, kMaxConditions = 32;
// JXS_EVAL_INNER_*, JXS_EVAL_OUTER_*
constexpr int kIdentity = 0, kAbs = 1, kSquare = 2, kExcess = 3;
constexpr int kInners = 4;
constexpr int kOuterIdentity = 0, kOuterExp = 1;
constexpr int kOuters = 2;
// kinds of a condition (JXS_EVAL_TERMINATED, JXS_EVAL_TRUNCATED) and the bits of `done` (JXS_DONE_*): bit = 1 << kind
constexpr int kKindTerminated = 0, kKindTruncated = 1;
constexpr int kCondKinds = 2;
constexpr unsigned kTerminated = 1u, kTruncated = 2u;

JXS_ENV_HD float magnitude(float x) { return fabsf(x); }
JXS_ENV_HD double magnitude(double x) { return fabs(x); }
JXS_ENV_HD float exponential(float x) { return expf(x); }
JXS_ENV_HD double exponential(double x) { return exp(x); }

// x of a slot from its raw word and the word of its target
template <typename T>
JXS_ENV_HD T slot_x(T raw, bool has_target, T target) {
  JXS_RAND_NO_CONTRACT
  return has_target ? raw - target : raw;
}

template <typename T>
JXS_ENV_HD T inner(int kind, T y) {
  JXS_RAND_NO_CONTRACT
  if (kind == kAbs) return magnitude(y);
  if (kind == kSquare) return y * y;
  if (kind == kExcess) {
    const T d = magnitude(y) - T(1);
    return d < T(0) ? T(0) : d;
  }
  return y;
}

template <typename T>
JXS_ENV_HD T outer(int kind, T s) {
  return kind == kOuterExp ? exponential(-s) : s;
}

// s of a term after one more slot: the sum is strictly sequential and never fused with the product of a square
template <typename T>
JXS_ENV_HD T accumulated(bool first, T s, T v) {
  JXS_RAND_NO_CONTRACT
  return first ? v : s + v;
}

// p of a term from the sum of its slots
template <typename T>
JXS_ENV_HD T weighted(int outer_kind, T s, T weight, T lo, T hi) {
  JXS_RAND_NO_CONTRACT
  const T w = weight * outer(outer_kind, s);
  return jxs_act::clamp(w, lo, hi);
}

// p of a term whose slots' words are y(first) .. y(first + count - 1)
template <typename T, typename Y>
JXS_ENV_HD T term_value(int first, int count, int inner_kind, int outer_kind, T weight, T lo, T hi, Y y) {
  T s = T(0);
  for (int d = first; d < first + count; ++d) s = accumulated(d == first, s, inner(inner_kind, y(d)));
  return weighted(outer_kind, s, weight, lo, hi);
}

template <typename T>
JXS_ENV_HD bool fires(T y, T lo, T hi) {
  return !(lo <= y && y <= hi);
}

// r of an environment from its K contributions p(0) .. p(K - 1), before the termination reward
template <typename T, typename P>
JXS_ENV_HD T total(int K, T reward_lo, T reward_hi, P p) {
  JXS_RAND_NO_CONTRACT
  T r = T(0);
  if (K > 0) r = p(0);
  for (int t = 1; t < K; ++t) r = r + p(t);
  return jxs_act::clamp(r, reward_lo, reward_hi);
}

template <typename T>
JXS_ENV_HD T terminal(T r, unsigned done, T termination_reward) {
  JXS_RAND_NO_CONTRACT
  return (done & kTerminated) ? r + termination_reward : r;
}

// the counter rule: the new counter, `done` gaining kTruncated when the episode is over.  (steps + 1 in unsigned
// arithmetic: a counter at INT32_MAX wraps to a negative number instead of overflowing)
JXS_ENV_HD int32_t counted(int32_t steps, int32_t max_steps, unsigned* done) {
  const int32_t n = (int32_t)((uint32_t)steps + 1u);
  if (n >= max_steps) *done |= kTruncated;
  return *done != 0 ? 0 : n;
}

// A table as the host holds it
template <typename T>
struct Table {
  int D, K, C;
  const int32_t* slots;    // [D][3] {kind, source, index} (jxs_obs::Slot)
  const int32_t* targets;  // [D][2] {source, row}, source -1: none; null: no slot has a target
  const T* offset;         // [D]
  const T* scale;          // [D]
  const int32_t* terms;    // [K][4] {first, count, inner, outer}
  const T* term_params;    // [K][3] {weight, lo, hi}
  const int32_t* conds;    // [C][2] {slot, kind}
  const T* cond_limits;    // [C][2] {lo, hi}
  T reward_lo, reward_hi, termination_reward;
};

template <typename T>
struct Result {
  T reward;
  unsigned done, fired;
  int32_t steps;
};

// Everything of one environment: row(r) is word r of its state rows, src(s, r) row r of its source s, term_out(t, p) takes
// the contribution of term t.  `counting`: the counter rule is applied to `steps`
template <typename T, typename Row, typename Src, typename TermOut>
JXS_ENV_HD Result<T> evaluate_env(const jxs_obs::Shape& sh, const Table<T>& tb, Row row, Src src, bool counting, int32_t steps, int32_t max_steps,
                                  TermOut term_out) {
  auto y = [&](int d) {
    const jxs_obs::Slot slot{tb.slots[3 * d], tb.slots[3 * d + 1], tb.slots[3 * d + 2]};
    const bool has_target = tb.targets != nullptr && tb.targets[2 * d] >= 0;
    const T raw = jxs_obs::slot_raw<T>(sh, slot, row, src);
    const T x = slot_x(raw, has_target, has_target ? src(tb.targets[2 * d], tb.targets[2 * d + 1]) : T(0));
    return jxs_obs::affine(x, tb.offset[d], tb.scale[d]);
  };
  T p[kMaxTerms];
  for (int t = 0; t < tb.K; ++t) {
    const int32_t* i = tb.terms + 4 * t;
    const T* w = tb.term_params + 3 * t;
    p[t] = term_value<T>(i[0], i[1], i[2], i[3], w[0], w[1], w[2], y);
    term_out(t, p[t]);
  }
  Result<T> res{T(0), 0u, 0u, steps};
  for (int c = 0; c < tb.C; ++c) {
    if (!fires(y(tb.conds[2 * c]), tb.cond_limits[2 * c], tb.cond_limits[2 * c + 1])) continue;
    res.fired |= 1u << c;
    res.done |= 1u << tb.conds[2 * c + 1];
  }
  if (counting) res.steps = counted(steps, max_steps, &res.done);
  res.reward = terminal(total<T>(tb.K, tb.reward_lo, tb.reward_hi, [&](int t) { return p[t]; }), res.done, tb.termination_reward);
  return res;
}

// a limit: no NaN, and infinite or finite in the block's type
template <typename T>
inline bool limit_ok(double v, T t) {
  return v == v && (v - v != 0.0 || jxs_obs::affine_ok(v, t));
}

// Validity of a table in double precision as the create call receives it (host only).  kOk, or the first error and the
// slot, term or condition it is in (-1: the table as a whole)
constexpr int kOk = 0, kBadWidth = 1, kBadSlot = 2, kBadTarget = 3, kBadTerm = 4, kBadRange = 5, kBadCondition = 6, kUnowned = 7, kNotFinite = 8,
              kBadLimits = 9;
struct Desc {
  long long D, K, C;
  const int32_t* slots;
  const int32_t* targets;
  const double* offset;  // null: 0
  const double* scale;   // null: 1
  const int32_t* terms;
  const double* term_params;
  const int32_t* conds;
  const double* cond_limits;
  double reward_lo, reward_hi, termination_reward;
};
template <typename T>
inline int table_error(const Desc& d, int n_rows, const int32_t* rows_s, T t, int* bad, int* slot_code) {
  *bad = -1, *slot_code = jxs_obs::kOk;
  if (d.D < 1 || d.D > kMaxSlots || d.K < 0 || d.K > kMaxTerms || d.C < 0 || d.C > kMaxConditions) return kBadWidth;
  if (d.slots == nullptr || (d.K > 0 && (d.terms == nullptr || d.term_params == nullptr)) || (d.C > 0 && (d.conds == nullptr || d.cond_limits == nullptr)))
    return kBadWidth;
  const int D = (int)d.D, K = (int)d.K, C = (int)d.C;
  for (int i = 0; i < D; ++i) {
    *bad = i;
    *slot_code = jxs_obs::slot_error(jxs_obs::Slot{d.slots[3 * i], d.slots[3 * i + 1], d.slots[3 * i + 2]}, n_rows, rows_s);
    if (*slot_code != jxs_obs::kOk) return kBadSlot;
    if (d.targets != nullptr && d.targets[2 * i] != -1) {
      const int s = d.targets[2 * i], r = d.targets[2 * i + 1];
      if (s < 0 || s >= jxs_obs::kSources || rows_s == nullptr || rows_s[s] <= 0 || r < 0 || r >= rows_s[s]) return kBadTarget;
    }
    if (!jxs_obs::affine_ok(d.offset != nullptr ? d.offset[i] : 0.0, t) || !jxs_obs::affine_ok(d.scale != nullptr ? d.scale[i] : 1.0, t)) return kNotFinite;
  }
  bool owned[kMaxSlots] = {};
  for (int k = 0; k < K; ++k) {
    *bad = k;
    const int32_t* i = d.terms + 4 * k;
    const double* w = d.term_params + 3 * k;
    if (i[2] < 0 || i[2] >= kInners || i[3] < 0 || i[3] >= kOuters) return kBadTerm;
    if (i[1] < 1 || i[0] < 0 || (long long)i[0] + i[1] > D) return kBadRange;
    for (int s = i[0]; s < i[0] + i[1]; ++s) {
      if (owned[s]) return kBadRange;
      owned[s] = true;
    }
    if (!jxs_obs::affine_ok(w[0], t)) return kNotFinite;
    if (!(w[1] <= w[2]) || !limit_ok(w[1], t) || !limit_ok(w[2], t)) return kBadLimits;
  }
  for (int c = 0; c < C; ++c) {
    *bad = c;
    const int s = d.conds[2 * c], kind = d.conds[2 * c + 1];
    if (kind < 0 || kind >= kCondKinds || s < 0 || s >= D || owned[s]) return kBadCondition;
    owned[s] = true;
    if (!(d.cond_limits[2 * c] <= d.cond_limits[2 * c + 1]) || !limit_ok(d.cond_limits[2 * c], t) || !limit_ok(d.cond_limits[2 * c + 1], t))
      return kBadLimits;
  }
  for (int i = 0; i < D; ++i)
    if (!owned[i]) {
      *bad = i;
      return kUnowned;
    }
  *bad = -1;
  if (!(d.reward_lo <= d.reward_hi) || !limit_ok(d.reward_lo, t) || !limit_ok(d.reward_hi, t)) return kBadLimits;
  if (!jxs_obs::affine_ok(d.termination_reward, t)) return kNotFinite;
  return kOk;
}

// The table as the kernel reads it: per slot its packed word (jxs_obs::pack_slot), its target word (-1, or source | row << 2),
// offset and scale; per term {first, count, inner, outer} and {weight, lo, hi}; per condition {slot, kind} and {lo, hi}
JXS_ENV_HD int32_t pack_target(int source, int row) { return source < 0 ? -1 : (int32_t)((uint32_t)source | ((uint32_t)row << 2)); }
JXS_ENV_HD int target_source(int32_t word) { return word & 3; }
JXS_ENV_HD int target_row(int32_t word) { return (int)((uint32_t)word >> 2); }

}  // namespace jxs_eval

#if !defined(__clang__)
#pragma GCC pop_options
#endif
