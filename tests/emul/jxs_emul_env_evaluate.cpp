// TEST INFRASTRUCTURE: host harness of the reward and termination flags (jxs_env_evaluate of jaxsim_amd/csrc/jxs_env.hip).
// It drives jxs_eval::evaluate_env of jaxsim_amd/csrc/jxs_env_evaluate.h -- the function the device kernel's pieces make up --
// over EVERY environment on the CPU, reading the tiled state and source blocks through the index functions of
// jxs_env_ops.h, so that tests/test_env_evaluate_cpu.py can compare it with the NumPy restatement
// (tests/env_evaluate_ref.py).  Built by tests/env_emul_lib.py with g++.
#include <cstdint>
#include <vector>

#include "jxs_env_evaluate.h"

namespace {

struct Outputs {
  void* reward;
  uint8_t* done;
  uint32_t* fired;
  void* terms;
  long long terms_ld;
  int32_t* steps;
  int max_steps;
};

template <typename T, typename R, typename TT>
void evaluate_all(const T* state, const T* const* sources, const int32_t* source_rows, const jxs_eval::Desc& d, const jxs_obs::Shape& sh, int N, int tile,
                  const Outputs& o) {
  const int D = (int)d.D, K = (int)d.K, C = (int)d.C;
  std::vector<T> offset(D), scale(D), term_params(3 * K + 1), cond_limits(2 * C + 1);
  for (int i = 0; i < D; ++i) offset[i] = (T)(d.offset ? d.offset[i] : 0.0), scale[i] = (T)(d.scale ? d.scale[i] : 1.0);
  for (int i = 0; i < 3 * K; ++i) term_params[i] = (T)d.term_params[i];
  for (int i = 0; i < 2 * C; ++i) cond_limits[i] = (T)d.cond_limits[i];
  const jxs_eval::Table<T> tb{D, K, C, d.slots, d.targets, offset.data(), scale.data(), d.terms, term_params.data(), d.conds, cond_limits.data(),
                              (T)d.reward_lo, (T)d.reward_hi, (T)d.termination_reward};
  for (long long env = 0; env < N; ++env) {
    auto row = [&](int r) { return state[jxs_env::word_of(env, r, sh.n_rows, tile)]; };
    auto src = [&](int s, int r) { return sources[s][jxs_env::word_of(env, r, source_rows[s], tile)]; };
    auto term_out = [&](int t, T p) {
      if (o.terms != nullptr) static_cast<TT*>(o.terms)[env * o.terms_ld + t] = (TT)p;
    };
    const jxs_eval::Result<T> res =
        jxs_eval::evaluate_env<T>(sh, tb, row, src, o.steps != nullptr, o.steps != nullptr ? o.steps[env] : 0, o.max_steps, term_out);
    if (o.reward != nullptr) static_cast<R*>(o.reward)[env] = (R)res.reward;
    if (o.done != nullptr) o.done[env] = (uint8_t)res.done;
    if (o.fired != nullptr) o.fired[env] = res.fired;
    if (o.steps != nullptr) o.steps[env] = res.steps;
  }
}

}  // namespace

extern "C" {

struct jxs_emul_eval_desc {
  int32_t D, K, C;
  const int32_t* slots;
  const int32_t* targets;
  const double* offset;
  const double* scale;
  const int32_t* terms;
  const double* term_params;
  const int32_t* conds;
  const double* cond_limits;
  double reward_lo, reward_hi, termination_reward;
};

static jxs_eval::Desc desc_of(const jxs_emul_eval_desc* d) {
  return jxs_eval::Desc{d->D, d->K, d->C, d->slots, d->targets, d->offset, d->scale, d->terms, d->term_params, d->conds, d->cond_limits,
                        d->reward_lo, d->reward_hi, d->termination_reward};
}

// kOk (0) or the error of jxs_eval::table_error, with the slot, term or condition it is in
int jxs_emul_evaluate_table_error(const jxs_emul_eval_desc* d, int n_rows, const int32_t* source_rows, int word_bytes, int* bad) {
  int slot_code;
  const jxs_eval::Desc dd = desc_of(d);
  return word_bytes == 4 ? jxs_eval::table_error(dd, n_rows, source_rows, 0.0f, bad, &slot_code) : jxs_eval::table_error(dd, n_rows, source_rows, 0.0, bad, &slot_code);
}

int32_t jxs_emul_evaluate_counted(int32_t steps, int32_t max_steps, unsigned* done) { return jxs_eval::counted(steps, max_steps, done); }

// -1: bad word sizes, -2: an invalid table, a null source the table reads, no output, terms_ld < K or steps without max_steps
int jxs_emul_env_evaluate(const void* state, const void* const* sources, const int32_t* source_rows, const jxs_emul_eval_desc* d, int n_rows, int n_joints,
                          int repr, int N, int tile, void* reward, int reward_word_bytes, uint8_t* done, uint32_t* fired, void* terms,
                          int terms_word_bytes, long long terms_ld, int32_t* steps, int max_steps, int word_bytes) {
  const jxs_eval::Desc dd = desc_of(d);
  int bad, slot_code;
  const int err = word_bytes == 4 ? jxs_eval::table_error(dd, n_rows, source_rows, 0.0f, &bad, &slot_code)
                                  : jxs_eval::table_error(dd, n_rows, source_rows, 0.0, &bad, &slot_code);
  if (err != jxs_eval::kOk) return -2;
  if ((reward == nullptr && done == nullptr) || (terms != nullptr && terms_ld < d->K) || (steps != nullptr && max_steps <= 0)) return -2;
  for (int i = 0; i < d->D; ++i) {
    if (d->slots[3 * i] == jxs_obs::kSourceRow && sources[d->slots[3 * i + 1]] == nullptr) return -2;
    if (d->targets != nullptr && d->targets[2 * i] >= 0 && sources[d->targets[2 * i]] == nullptr) return -2;
  }
  const jxs_obs::Shape sh{n_rows, n_joints, repr};
  const Outputs o{reward, done, fired, terms, terms_ld, steps, max_steps};
  const int rb = reward != nullptr ? reward_word_bytes : word_bytes, tb = terms != nullptr ? terms_word_bytes : word_bytes;
  if (word_bytes == 4 && rb == 4 && tb == 4)
    evaluate_all<float, float, float>(static_cast<const float*>(state), reinterpret_cast<const float* const*>(sources), source_rows, dd, sh, N, tile, o);
  else if (word_bytes == 8 && rb == 8 && tb == 8)
    evaluate_all<double, double, double>(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, dd, sh, N, tile, o);
  else if (word_bytes == 8 && rb == 4 && tb == 8)
    evaluate_all<double, float, double>(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, dd, sh, N, tile, o);
  else if (word_bytes == 8 && rb == 8 && tb == 4)
    evaluate_all<double, double, float>(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, dd, sh, N, tile, o);
  else if (word_bytes == 8 && rb == 4 && tb == 4)
    evaluate_all<double, float, float>(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, dd, sh, N, tile, o);
  else
    return -1;
  return 0;
}

}  // extern "C"
