// TEST INFRASTRUCTURE: host harness of the per-environment operations (jxs_env_select, jxs_env_copy, jxs_env_flags of
// jaxsim_amd/csrc/jxs_env.hip).  It drives the index functions of jaxsim_amd/csrc/jxs_env_ops.h -- the ones the device
// kernels are loops around -- over EVERY word of a block on the CPU, so that tests/test_env_ops_cpu.py can compare them
// with the NumPy restatement (tests/env_ops_ref.py) bit for bit.  Built by tests/env_ops_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "jxs_env_ops.h"

namespace {

// out word = a's or b's, by the column's mask byte; every word of the storage, padding included
void select_words(const uint8_t* mask, const unsigned char* a, const unsigned char* b, unsigned char* out, int rows, int N, int tile, int wb) {
  const long long total = jxs_env::block_words(rows, N, tile);
  for (long long w = 0; w < total; ++w) {
    const jxs_env::WordPos p = jxs_env::split_word(w, rows, tile);
    const long long env = jxs_env::env_of(p.tile, p.col, tile);
    // the two-step form of the kernel must agree with the one-step form
    const long long in_tile = w - p.tile * jxs_env::tile_words(rows, tile);
    if (jxs_env::col_of(in_tile, tile) != p.col || (!jxs_env::is_padding(env, N) && jxs_env::word_of(env, p.row, rows, tile) != w)) {
      std::memset(out, 0xEE, (size_t)total * wb);  // (shows as a mismatch of the whole block)
      return;
    }
    unsigned char word[8];
    std::memcpy(word, (jxs_env::select_takes_a(mask, env, N) ? a : b) + (size_t)w * wb, wb);
    std::memcpy(out + (size_t)w * wb, word, wb);
  }
}

template <typename T>
void flags_words(const T* state, int rows, int row_quat, int N, int tile, uint8_t* out) {
  std::vector<uint8_t> bad(N, 0);
  const long long total = jxs_env::block_words(rows, N, tile);
  for (long long w = 0; w < total; ++w) {
    const jxs_env::WordPos p = jxs_env::split_word(w, rows, tile);
    const long long env = jxs_env::env_of(p.tile, p.col, tile);
    if (jxs_env::is_padding(env, N)) continue;
    const volatile T v = state[w];
    if (!(v - v == T(0))) bad[env] = 1;
  }
  for (long long env = 0; env < N; ++env) {
    T q2 = 0;
    bool nan_q = false;
    for (int k = 0; k < 4; ++k) {
      const volatile T v = state[jxs_env::word_of(env, row_quat + k, rows, tile)];
      nan_q = nan_q || (v != v);
      const volatile T sq = v * v;  // (rounded to T before the sum: no excess precision, no contraction)
      q2 = q2 + sq;
    }
    const T d = q2 > T(1) ? q2 - T(1) : T(1) - q2;
    int f = bad[env] ? jxs_env::kFlagNonFinite : 0;
    if (!nan_q && !(d <= T(1e-8) + T(1e-5))) f |= jxs_env::kFlagQuatNotUnit;
    out[env] = (uint8_t)f;
  }
}

}  // namespace

extern "C" {

int jxs_emul_env_select(const uint8_t* mask, const void* a, const void* b, void* out, int rows, int N, int tile, int word_bytes) {
  if (word_bytes != 4 && word_bytes != 8) return -1;
  select_words(mask, (const unsigned char*)a, (const unsigned char*)b, (unsigned char*)out, rows, N, tile, word_bytes);
  return 0;
}

// the loop of jxs_env_copy_kernel over its flat range K * rows
int jxs_emul_env_copy(const void* src, int src_N, int src_tile, const int32_t* src_idx, void* dst, int dst_N, int dst_tile,
                      const int32_t* dst_idx, int rows, int K, int word_bytes) {
  if (word_bytes != 4 && word_bytes != 8) return -1;
  const long long total = (long long)K * rows;
  for (long long i = 0; i < total; ++i) {
    const long long k = i / rows;
    const int row = (int)(i % rows);
    long long se, de;
    if (!jxs_env::copy_pair(src_idx, dst_idx, k, src_N, dst_N, &se, &de)) continue;
    const long long sw = jxs_env::copy_src_word(se, row, rows, src_tile), dw = jxs_env::copy_dst_word(de, row, rows, dst_tile);
    if (sw < 0 || sw >= jxs_env::block_words(rows, src_N, src_tile) || dw < 0 || dw >= jxs_env::block_words(rows, dst_N, dst_tile)) return -2;
    std::memcpy((unsigned char*)dst + (size_t)dw * word_bytes, (const unsigned char*)src + (size_t)sw * word_bytes, word_bytes);
  }
  return 0;
}

int jxs_emul_env_flags(const void* state, int rows, int row_quat, int N, int tile, int word_bytes, uint8_t* out) {
  if (word_bytes == 4) flags_words((const float*)state, rows, row_quat, N, tile, out);
  else if (word_bytes == 8) flags_words((const double*)state, rows, row_quat, N, tile, out);
  else return -1;
  return 0;
}

int jxs_emul_env_access_bytes(unsigned long long address_bits, int rows, int tile, int word_bytes) {
  return jxs_env::access_bytes(address_bits, rows, tile, word_bytes);
}

int jxs_emul_env_shift_for(int N, int tile_shift, int want) { return jxs_env::env_shift_for(N, tile_shift, want); }

long long jxs_emul_env_block_words(int rows, long long N, int tile) { return jxs_env::block_words(rows, N, tile); }

long long jxs_emul_env_word_of(long long env, int row, int rows, int tile) { return jxs_env::word_of(env, row, rows, tile); }

}  // extern "C"
