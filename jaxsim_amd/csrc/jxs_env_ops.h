// Index arithmetic of the per-environment operations on the tiled storage (jxs_env_select, jxs_env_copy,
// jxs_env_flags in jxs_api.hip): which environment a word of a block belongs to, where a word of an environment
// lies, which columns are padding, which entries of an index list are copied.  Plain integer functions for host and
// device: the kernels are loops around them, and tests/emul/jxs_emul_env_ops.cpp drives the same functions over
// every word on the CPU.
//
// Storage (jaxsim_amd/state.py tile_block): a logical [rows][N] array is kept as [ceil(N/T)][rows][T], T = `tile`
// environments interleaved per row; the last tile is padded to T columns.  T = 1 is the environment-major
// layout [N][rows].  Offsets are counted in words (one float or double) and held in 64 bits: rows * N words pass
// 2^31 for large batches.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JXS_ENV_HD __host__ __device__ inline
#else
#define JXS_ENV_HD inline
#endif

namespace jxs_env {

// bits of the byte jxs_env_flags writes per environment
constexpr int kFlagNonFinite = 1;    // some word of the environment is NaN or infinite
constexpr int kFlagQuatNotUnit = 2;  // no NaN in the quaternion, and | |q|^2 - 1 | > 1e-8 + 1e-5

struct WordPos {
  long long tile;  // tile index
  int row;         // row of the logical array
  int col;         // column inside the tile, 0 .. T-1
};

JXS_ENV_HD long long n_tiles(long long N, int tile) { return (N + tile - 1) / tile; }

// words of one tile: its rows * T words are contiguous
JXS_ENV_HD long long tile_words(int rows, int tile) { return (long long)rows * tile; }

// words of the whole block, padding included
JXS_ENV_HD long long block_words(int rows, long long N, int tile) { return n_tiles(N, tile) * tile_words(rows, tile); }

// flat word of the storage -> (tile, row, column)
JXS_ENV_HD WordPos split_word(long long word, int rows, int tile) {
  const long long per_tile = tile_words(rows, tile);
  const long long in_tile = word % per_tile;
  return WordPos{word / per_tile, (int)(in_tile / tile), (int)(in_tile % tile)};
}

// word inside its tile -> column (the row is in_tile / tile)
JXS_ENV_HD int col_of(long long in_tile, int tile) { return (int)(in_tile % tile); }

// (tile, column) -> environment.  May be >= N: a padding column of the last tile
JXS_ENV_HD long long env_of(long long tile_index, int col, int tile) { return tile_index * tile + col; }

// the padding rule: columns at or beyond N exist in the storage and belong to no environment
JXS_ENV_HD bool is_padding(long long env, long long N) { return env >= N; }

// (environment, row) -> flat word of the storage
JXS_ENV_HD long long word_of(long long env, int row, int rows, int tile) {
  return ((env / tile) * rows + row) * tile + env % tile;
}

// jxs_env_select: does this column take a's words?  Padding columns never do, and `mask` is not read for them
JXS_ENV_HD bool select_takes_a(const uint8_t* mask, long long env, long long N) {
  return !is_padding(env, N) && mask[env] != 0;
}

// jxs_env_copy: entry k of the lists as (source environment, destination environment).  A null list means k itself.
// False = the entry is skipped entirely: one of the two is outside its block
JXS_ENV_HD bool copy_pair(const int32_t* src_idx, const int32_t* dst_idx, long long k, long long src_N, long long dst_N,
                          long long* src_env, long long* dst_env) {
  const long long s = src_idx != nullptr ? (long long)src_idx[k] : k;
  const long long d = dst_idx != nullptr ? (long long)dst_idx[k] : k;
  *src_env = s;
  *dst_env = d;
  return s >= 0 && s < src_N && d >= 0 && d < dst_N;
}

// jxs_env_copy works on the flat range [0, K * rows): entry k = i / rows, row = i % rows, so that neighbouring
// threads touch neighbouring rows (contiguous where a side is environment-major).  The word read and the word
// written, each in its own tiling:
JXS_ENV_HD long long copy_src_word(long long src_env, int row, int rows, int src_tile) { return word_of(src_env, row, rows, src_tile); }
JXS_ENV_HD long long copy_dst_word(long long dst_env, int row, int rows, int dst_tile) { return word_of(dst_env, row, rows, dst_tile); }

// Widest access, in bytes out of {16, 8, 4}, that every tile span of a block allows: the span of one tile
// (rows * T words of `word_bytes`) and the address of the block must both be multiples of it.  Never below
// `word_bytes` for a block aligned to its words.  (The humanoid's fp32 tile is 155 * 2 * 4 = 1240 bytes: 8.)
JXS_ENV_HD int access_bytes(unsigned long long address_bits, int rows, int tile, int word_bytes) {
  const unsigned long long span = (unsigned long long)tile_words(rows, tile) * (unsigned)word_bytes;
  for (int a = 16; a > word_bytes; a >>= 1)
    if (span % a == 0 && address_bits % a == 0) return a;
  return word_bytes;
}

// Environments per wave of jxs_env_observe, jxs_env_act, jxs_env_evaluate and jxs_env_contacts (host only), E = 2^shift with T <= E <= max(T, 32), T = 2^tile_shift:
// as many as still leave the chip 8192 waves (256 CUs x 4 SIMDs x 8), so that what a wave reads once (the table, the derived
// values' prologue) is shared by more environments at large N, while a small batch is spread over as many waves as it has
// tiles.  `want` > 0 (the launcher's developer knob) asks for at least that many instead, within the same limits.
// Measured on the humanoid.  The 60-wide observation (profiles/env_observe.txt): at N = 65 536 fastest with 8 environments
// per wave (about 18.5 / 13 / 10.7 / 11.8 / 14.7 us with 2 / 4 / 8 / 16 / 32), at N = 1024 with one tile per wave (32
// environments per wave take twice as long).  The torques (profiles/env_act.txt): at N = 65 536 a wave of 4, 8 or 16
// environments takes 7.2 .. 7.4 us, one of 2 or 32 about 11 us; at N = 1024 everything up to 8 is one launch interval (3.6 us).
// The reward and termination flags (jxs_env_evaluate, profiles/env_evaluate.txt): at N = 65 536 about 123 / 70 / 47.7 / 44.7 / 46.0 us
// with 2 / 4 / 8 / 16 / 32, at N = 1024 18.9 .. 19.2 us up to 8 and 25.6 / 28.3 us with 16 / 32: the same rule, within 7 % of the best.
// The contact sensors (jxs_env_contacts, profiles/env_contact.txt) give their points lanes, so one tile fills a wave: their launcher passes
// `want` = T, one tile per wave whatever N (8 per wave take 1.5 x the time of 2 or 4 at N = 65 536, 16 and 32 take 2.8 x).
inline int env_shift_for(int N, int tile_shift, int want) {
  const int max_shift = tile_shift > 5 ? tile_shift : 5;
  int shift = tile_shift;
  if (want > 0) {
    while (shift < max_shift && (1 << shift) < want) ++shift;
  } else {
    while (shift < max_shift && ((long long)N >> (shift + 1)) >= 8192) ++shift;
  }
  return shift;
}

}  // namespace jxs_env
