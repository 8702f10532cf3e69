// TEST INFRASTRUCTURE: host harness of the random reset (jxs_env_randomize of jaxsim_amd/csrc/jxs_env.hip).  It drives
// the functions of jaxsim_amd/csrc/jxs_env_random.h -- the ones the device kernel is a loop around -- over EVERY word of
// a block on the CPU, so that tests/test_env_random_cpu.py can compare them with the NumPy restatement
// (tests/env_random_ref.py).  Built by tests/env_random_emul.py with g++.
#include <cstdint>
#include <cstring>

#include "jxs_env_random.h"

namespace {

template <typename T>
void randomize_words(const uint8_t* mask, T* state, int rows, int N, int tile, const jxs_rand::Shape& sh, const T* bounds, uint64_t seed,
                     uint64_t draw, long long first_env) {
  const long long total = jxs_env::block_words(rows, N, tile);
  for (long long w = 0; w < total; ++w) {
    const jxs_env::WordPos p = jxs_env::split_word(w, rows, tile);
    const long long env = jxs_env::env_of(p.tile, p.col, tile);
    if (jxs_env::is_padding(env, N)) continue;          // (the mask is not read for a padding column)
    if (mask != nullptr && mask[env] == 0) continue;
    const T v = jxs_rand::row_value<T>(sh, p.row, bounds, seed, draw, (uint32_t)(first_env + env));
    std::memcpy(&state[w], &v, sizeof(T));
  }
}

}  // namespace

extern "C" {

void jxs_emul_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { jxs_rand::philox4x32_10(ctr, key, out); }

// in place on `state`; mask may be null (every environment).  -1: bad word size, -2: first_env + N outside 32 bits
int jxs_emul_env_randomize(const uint8_t* mask, void* state, int rows, int N, int tile, int n_joints, int floating, int repr,
                           const void* bounds, uint64_t seed, uint64_t draw, long long first_env, int word_bytes) {
  if (!jxs_rand::env_range_ok(first_env, N)) return -2;
  const jxs_rand::Shape sh{n_joints, floating, repr};
  if (word_bytes == 4) randomize_words(mask, (float*)state, rows, N, tile, sh, (const float*)bounds, seed, draw, first_env);
  else if (word_bytes == 8) randomize_words(mask, (double*)state, rows, N, tile, sh, (const double*)bounds, seed, draw, first_env);
  else return -1;
  return 0;
}

int jxs_emul_env_random_variables(int n_joints) { return jxs_rand::n_variables(n_joints); }

}  // extern "C"
