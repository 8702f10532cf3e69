// TEST INFRASTRUCTURE: host harness of the policy observation (jxs_env_observe of jaxsim_amd/csrc/jxs_env.hip).  It drives
// jxs_obs::slot_value of jaxsim_amd/csrc/jxs_env_observe.h -- the function the device kernel's pieces make up -- over EVERY
// word of the tensor on the CPU, reading the tiled state and source blocks through the index functions of jxs_env_ops.h, so
// that tests/test_env_observe_cpu.py can compare it with the NumPy restatement (tests/env_observe_ref.py).  Built by
// tests/env_observe_emul.py with g++.
#include <cstdint>
#include <cstring>

#include "jxs_env_observe.h"

namespace {

// out[N][out_ld]: columns < D of every row are written, the others left alone
template <typename T, typename O>
void observe_words(const T* state, const T* const* sources, const int32_t* source_rows, const int32_t* slots, const T* offset, const T* scale, int D,
                   const jxs_obs::Shape& sh, int N, int tile, O* out, long long out_ld) {
  for (long long env = 0; env < N; ++env) {
    auto row = [&](int r) { return state[jxs_env::word_of(env, r, sh.n_rows, tile)]; };
    auto src = [&](int s, int r) { return sources[s][jxs_env::word_of(env, r, source_rows[s], tile)]; };
    for (int d = 0; d < D; ++d) {
      const jxs_obs::Slot slot{slots[3 * d], slots[3 * d + 1], slots[3 * d + 2]};
      out[env * out_ld + d] = (O)jxs_obs::slot_value<T>(sh, slot, offset[d], scale[d], row, src);
    }
  }
}

}  // namespace

extern "C" {

// kOk (0) or the error of jxs_obs::table_error, with the slot it is in
int jxs_emul_observe_table_error(const int32_t* slots, long long D, int n_rows, const int32_t* source_rows, int* bad_slot) {
  return jxs_obs::table_error(slots, D, n_rows, source_rows, bad_slot);
}

int jxs_emul_observe_affine_ok(double v, int word_bytes) { return word_bytes == 4 ? jxs_obs::affine_ok(v, 0.0f) : jxs_obs::affine_ok(v, 0.0); }

unsigned jxs_emul_observe_derived_used(const int32_t* slots, int D, int repr) { return jxs_obs::derived_used(slots, D, repr); }

// offset and scale in the block's type.  -1: bad word sizes, -2: an invalid table or a null source the table reads
int jxs_emul_env_observe(const void* state, const void* const* sources, const int32_t* source_rows, const int32_t* slots, const void* offset,
                         const void* scale, int D, int n_rows, int n_joints, int repr, int N, int tile, void* out, long long out_ld, int word_bytes,
                         int out_word_bytes) {
  int bad;
  if (jxs_obs::table_error(slots, D, n_rows, source_rows, &bad) != jxs_obs::kOk || out_ld < D) return -2;
  for (int d = 0; d < D; ++d)
    if (slots[3 * d] == jxs_obs::kSourceRow && sources[slots[3 * d + 1]] == nullptr) return -2;
  const jxs_obs::Shape sh{n_rows, n_joints, repr};
  if (word_bytes == 4 && out_word_bytes == 4)
    observe_words(static_cast<const float*>(state), reinterpret_cast<const float* const*>(sources), source_rows, slots, static_cast<const float*>(offset),
                  static_cast<const float*>(scale), D, sh, N, tile, static_cast<float*>(out), out_ld);
  else if (word_bytes == 8 && out_word_bytes == 8)
    observe_words(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, slots, static_cast<const double*>(offset),
                  static_cast<const double*>(scale), D, sh, N, tile, static_cast<double*>(out), out_ld);
  else if (word_bytes == 8 && out_word_bytes == 4)
    observe_words(static_cast<const double*>(state), reinterpret_cast<const double* const*>(sources), source_rows, slots, static_cast<const double*>(offset),
                  static_cast<const double*>(scale), D, sh, N, tile, static_cast<float*>(out), out_ld);
  else
    return -1;
  return 0;
}

}  // extern "C"
