// TEST INFRASTRUCTURE: host harness of the action-to-torque law (jxs_env_act of jaxsim_amd/csrc/jxs_env.hip).  It drives
// jxs_act::torque_word of jaxsim_amd/csrc/jxs_env_act.h -- the function the device kernel calls per word -- over EVERY word
// of the tiled torque block on the CPU, reading the tiled state and feed-forward blocks through the index functions of
// jxs_env_ops.h, so that tests/test_env_act_cpu.py can compare it with the NumPy restatement (tests/env_act_ref.py).  The
// padding columns of the last tile are written as zero.  Built by tests/env_act_emul.py with g++.
#include <cstdint>
#include <cstring>

#include "jxs_env_act.h"

namespace {

template <typename T, typename AT>
void act_words(const T* state, const AT* actions, long long act_ld, const int32_t* joints, const double* params, int n, int n_rows, const T* ff, T* out,
               int N, int tile) {
  const long long padded = jxs_env::n_tiles(N, tile) * tile;
  for (long long env = 0; env < padded; ++env)
    for (int j = 0; j < n; ++j) {
      T& word = out[jxs_env::word_of(env, j, n, tile)];
      if (jxs_env::is_padding(env, N)) {
        word = T(0);
        continue;
      }
      T p[jxs_act::kParams];
      for (int k = 0; k < jxs_act::kParams; ++k) p[k] = static_cast<T>(params[jxs_act::kParams * j + k]);
      const int mode = joints[2 * j], column = joints[2 * j + 1];
      const T a = column < 0 ? T(0) : (T)actions[env * act_ld + column];
      const T q = state[jxs_env::word_of(env, jxs_act::row_q(n) + j, n_rows, tile)];
      const T qd = state[jxs_env::word_of(env, jxs_act::row_qd(n) + j, n_rows, tile)];
      const T f = ff != nullptr ? ff[jxs_env::word_of(env, j, n, tile)] : T(0);
      word = jxs_act::torque_word(mode, column, a, p, q, qd, ff != nullptr, f);
    }
}

}  // namespace

extern "C" {

// kOk (0) or the error of jxs_act::table_error, with the joint it is in
int jxs_emul_act_table_error(const int32_t* joints, const double* params, long long n, long long A, int word_bytes, int* bad_joint) {
  return word_bytes == 4 ? jxs_act::table_error(joints, params, n, A, 0.0f, bad_joint) : jxs_act::table_error(joints, params, n, A, 0.0, bad_joint);
}

int jxs_emul_act_finite_ok(double v, int word_bytes) { return word_bytes == 4 ? jxs_act::finite_ok(v, 0.0f) : jxs_act::finite_ok(v, 0.0); }
int jxs_emul_act_limit_ok(double v, int word_bytes) { return word_bytes == 4 ? jxs_act::limit_ok(v, 0.0f) : jxs_act::limit_ok(v, 0.0); }
int jxs_emul_act_targets_ok(double lo, double hi, int word_bytes) {
  return word_bytes == 4 ? jxs_act::targets_ok(lo, hi, 0.0f) : jxs_act::targets_ok(lo, hi, 0.0);
}
// pack_joint and back: 0 when mode and column survive
int jxs_emul_act_pack_roundtrip(int mode, int column) {
  const int32_t code = jxs_act::pack_joint(mode, column);
  return jxs_act::packed_mode(code) == mode && jxs_act::packed_column(code) == column ? 0 : 1;
}

// -1: bad word sizes, -2: an invalid table, act_ld < A or null actions the table reads
int jxs_emul_env_act(const void* state, const void* actions, long long act_ld, int A, const int32_t* joints, const double* params, int n, int n_rows,
                     const void* ff, void* out, int N, int tile, int word_bytes, int act_word_bytes) {
  int bad;
  const int err = word_bytes == 4 ? jxs_act::table_error(joints, params, n, A, 0.0f, &bad) : jxs_act::table_error(joints, params, n, A, 0.0, &bad);
  if (err != jxs_act::kOk || act_ld < A) return -2;
  for (int j = 0; j < n; ++j)
    if (joints[2 * j + 1] >= 0 && actions == nullptr) return -2;
  if (word_bytes == 4 && act_word_bytes == 4)
    act_words(static_cast<const float*>(state), static_cast<const float*>(actions), act_ld, joints, params, n, n_rows, static_cast<const float*>(ff),
              static_cast<float*>(out), N, tile);
  else if (word_bytes == 8 && act_word_bytes == 8)
    act_words(static_cast<const double*>(state), static_cast<const double*>(actions), act_ld, joints, params, n, n_rows, static_cast<const double*>(ff),
              static_cast<double*>(out), N, tile);
  else if (word_bytes == 8 && act_word_bytes == 4)
    act_words(static_cast<const double*>(state), static_cast<const float*>(actions), act_ld, joints, params, n, n_rows, static_cast<const double*>(ff),
              static_cast<double*>(out), N, tile);
  else
    return -1;
  return 0;
}

}  // extern "C"
