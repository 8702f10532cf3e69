// The per-environment operations of the C ABI (include/jaxsim_amd.h: jxs_env_*, jxs_observation_*, jxs_action_*,
// jxs_evaluation_*, jxs_contact_sensors_*): their device tables, kernels and entry points.  The laws the kernels evaluate are
// the jxs_env_*.h headers, shared with the host harness of the tests; models, error string and knobs are jxs_host.h.
#include <algorithm>
#include <type_traits>

#include "jxs_env_act.h"
#include "jxs_env_contact.h"
#include "jxs_env_evaluate.h"
#include "jxs_env_observe.h"
#include "jxs_env_ops.h"
#include "jxs_env_random.h"
#include "jxs_host.h"

using namespace jxs_host;

// an immutable observation table on the device (jxs_observation_create): per slot its packed word (jxs_obs::pack_slot),
// offset and scale, in one allocation [codes | offset | scale]
struct jxs_observation {
  int dtype = JXS_F32;
  int D = 0, n_rows = 0, n_joints = 0;
  int32_t source_rows[jxs_obs::kSources] = {0, 0, 0, 0};
  unsigned sources_used = 0;         // bit s: some slot reads source s
  unsigned derived_used[3] = {0, 0, 0};  // per JXS_REPR_*: the derived values a launch computes (jxs_obs::derived_used)
  void* table = nullptr;             // device
  size_t offset_at = 0, scale_at = 0;  // bytes from `table`
};

// an immutable action table on the device (jxs_action_create): per joint its packed word (jxs_act::pack_joint) and its
// eight parameters (jxs_act::Params), in one allocation [codes | params]
struct jxs_action {
  int dtype = JXS_F32;
  int A = 0, n_rows = 0, n_joints = 0;
  bool reads_actions = false;  // some joint has a column
  void* table = nullptr;       // device
  size_t params_at = 0;        // bytes from `table`
};

// an immutable reward and termination table on the device (jxs_evaluation_create), in one allocation: per slot its packed
// word (jxs_obs::pack_slot), target word (jxs_eval::pack_target), offset and scale; per term {first, count, inner, outer} and
// {weight, lo, hi}; per condition {slot, kind} and {lo, hi}
struct jxs_evaluation {
  int dtype = JXS_F32;
  int D = 0, K = 0, C = 0, n_rows = 0, n_joints = 0;
  int32_t source_rows[jxs_obs::kSources] = {0, 0, 0, 0};
  unsigned sources_used = 0;             // bit s: some slot or target reads source s
  unsigned derived_used[3] = {0, 0, 0};  // per JXS_REPR_*: the derived values a launch computes (jxs_obs::derived_used)
  double reward_lo = 0, reward_hi = 0, termination_reward = 0;
  void* table = nullptr;  // device
  size_t targets_at = 0, offset_at = 0, scale_at = 0, terms_at = 0, term_params_at = 0, conds_at = 0, cond_limits_at = 0;  // bytes from `table`
};

// an immutable contact-sensor table on the device (jxs_contact_sensors_create), in one allocation: per group {first, count},
// per entry its parent link and L_p in the model's dtype
struct jxs_contact_sensors {
  int dtype = JXS_F32;
  int G = 0, P = 0, n_rows = 0, n_joints = 0, n_links = 0;
  void* table = nullptr;               // device
  size_t parent_at = 0, points_at = 0;  // bytes from `table`
};

// ---- the episode loop around `step`: reset, pick and flag environments of a batch on the device (the index arithmetic
// is jxs_env_ops.h, shared with the host harness of the tests) -------------------------------------------------------
template <int A>
struct alignas(A) EnvPack {
  uint32_t u[A / 4];
};

// out[:, e] = mask[e] ? a[:, e] : b[:, e].  One wave per tile, four tiles per workgroup: the wave reads the T mask bytes
// of its tile first (one ballot), and when none is set and the call is in place (out == b) it returns: a wave-uniform
// exit that has cost the mask read only, no state load and no store.  Otherwise its lanes run over the contiguous
// rows * T words of the tile in accesses of A bytes, each word of an access chosen by the mask bit of its column.
// In place, an access none of whose words is taken is skipped too; an access all of whose words are taken loads a only.
//
// Access width A: the widest of 16, 8, 4 bytes that divides the byte span of ONE tile and the three block addresses
// (jxs_env::access_bytes), because every tile starts at a multiple of that span.  The humanoid's fp32 tile is
// 155 rows * 2 columns * 4 bytes = 1240 bytes: a multiple of 8, not of 16, so it runs with 8-byte accesses
// (two fp32 words of one row); a 16-byte access would straddle a 16-byte line in every odd tile.  fp64 words are 8 bytes,
// A is 8 or 16.  WB = bytes of a word.  Words move as bits (integer registers): NaN payloads, -0, denormals survive.
template <int A, int WB>
__global__ void __launch_bounds__(256) jxs_env_select_kernel(const uint8_t* mask, const unsigned char* a, const unsigned char* b,
                                                             unsigned char* out, int rows, int N, int tile, long long tiles) {
  constexpr int WPA = A / WB, UPW = WB / 4;  // words per access, 32-bit units per word
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tiles) return;  // (wave-uniform)
  const bool inplace = out == b;
  const bool narrow = tile <= 64;  // the tile's mask fits one ballot; wider tiles read the mask byte per word
  unsigned long long bits = 0;
  bool any;
  if (narrow) {
    bits = __ballot(lane < tile && jxs_env::select_takes_a(mask, jxs_env::env_of(t, lane, tile), N));
    any = bits != 0;
  } else {
    bool m = false;
    for (int c = lane; c < tile; c += 64) m = m || jxs_env::select_takes_a(mask, jxs_env::env_of(t, c, tile), N);
    any = __ballot(m) != 0;
  }
  if (inplace && !any) return;
  // (words inside a tile are counted in 32 bits -- the host refuses a tile of 2^30 words --: the column of a word is a
  // remainder by the run-time `tile`, and a 64-bit remainder costs the lanes more than the copy itself)
  const int per_tile = (int)jxs_env::tile_words(rows, tile);
  const int n_acc = per_tile / WPA;  // (the host chose A so that this is exact)
  const size_t base = (size_t)t * (size_t)per_tile * WB;
  for (int i = lane; i < n_acc; i += 64) {
    bool take[WPA], some = false, all = true;
#pragma unroll
    for (int j = 0; j < WPA; ++j) {
      const int col = jxs_env::col_of(i * WPA + j, tile);
      take[j] = narrow ? ((bits >> col) & 1ull) != 0 : jxs_env::select_takes_a(mask, jxs_env::env_of(t, col, tile), N);
      some = some || take[j];
      all = all && take[j];
    }
    if (inplace && !some) continue;
    const size_t off = base + (size_t)i * A;
    EnvPack<A> v;
    if (all) {
      v = *reinterpret_cast<const EnvPack<A>*>(a + off);
    } else {
      v = *reinterpret_cast<const EnvPack<A>*>(b + off);
      if (some) {
        const EnvPack<A> va = *reinterpret_cast<const EnvPack<A>*>(a + off);
#pragma unroll
        for (int j = 0; j < WPA; ++j)
#pragma unroll
          for (int u = 0; u < UPW; ++u)
            if (take[j]) v.u[j * UPW + u] = va.u[j * UPW + u];
      }
    }
    *reinterpret_cast<EnvPack<A>*>(out + off) = v;
  }
}

// Environment src_idx[k] of `src` -> environment dst_idx[k] of `dst`, each block in its own tiling (tile 1 =
// environment-major).  One thread per (k, row) of the flat range K * rows, rows fastest.  An entry with an index outside
// its block is skipped whole (jxs_env::copy_pair): nothing outside the two blocks is read or written.
template <typename W>
__global__ void __launch_bounds__(256) jxs_env_copy_kernel(const W* src, int src_N, int src_tile, const int32_t* src_idx, W* dst, int dst_N,
                                                           int dst_tile, const int32_t* dst_idx, int rows, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long k = i / rows;
  const int row = (int)(i % rows);
  long long se, de;
  if (!jxs_env::copy_pair(src_idx, dst_idx, k, src_N, dst_N, &se, &de)) return;
  dst[jxs_env::copy_dst_word(de, row, rows, dst_tile)] = src[jxs_env::copy_src_word(se, row, rows, src_tile)];
}

// One byte per environment: bit 0 = some word NaN or infinite (the rule of counts3[2] of jxs_validate_kernel), bit 1 =
// no NaN in the quaternion and its squared norm off 1 by more than 1e-8 + 1e-5 (counts3[1]).  One wave per tile, its lanes
// over the contiguous words of the tile: `tile` divides 64, so a lane stays in the column lane % tile over all its words,
// and the columns are joined by a butterfly over the lanes of equal lane % tile.  Lane c < tile then evaluates the
// quaternion rule of column c in the summation order of jxs_validate_kernel (four words the wave has just read) and is
// the only writer of that environment's byte.  Padding columns are read and never reported.
template <typename T>
__global__ void __launch_bounds__(256) jxs_env_flags_kernel(const T* state, int rows, int row_quat, int tile, int N, long long tiles,
                                                            uint8_t* out) {
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tiles) return;  // (wave-uniform)
  const int per_tile = (int)jxs_env::tile_words(rows, tile);  // (the host refuses a tile of 2^30 words)
  const T* tp = state + (size_t)t * (size_t)per_tile;
  const long long env = jxs_env::env_of(t, lane, tile);
  const bool writer = lane < tile && !jxs_env::is_padding(env, N);
  // the writer's four quaternion words are asked for first, so that they travel with the words of the sweep below
  T q[4] = {T(0), T(0), T(0), T(0)};
  if (writer)
    for (int k = 0; k < 4; ++k) q[k] = tp[(row_quat + k) * tile + lane];
  int bad = 0;
  for (int w0 = 0; w0 < per_tile; w0 += 64) {
    const int w = w0 + lane;
    if (w < per_tile) {
      const T v = tp[w];
      bad |= !(v - v == T(0));  // NaN or infinity
    }
  }
  for (int o = tile; o < 64; o <<= 1) bad |= __shfl_xor(bad, o);
  if (!writer) return;
  T q2 = 0;
  bool nan_q = false;
  for (int k = 0; k < 4; ++k) {
    const T v = q[k];
    nan_q = nan_q || (v != v);
    q2 += v * v;
  }
  const T d = q2 > T(1) ? q2 - T(1) : T(1) - q2;
  int flags = bad ? jxs_env::kFlagNonFinite : 0;
  if (!nan_q && !(d <= T(1e-8) + T(1e-5))) flags |= jxs_env::kFlagQuatNotUnit;
  out[env] = (uint8_t)flags;
}

// A freshly sampled state into the environments the mask names, in place (the sampler is jxs_env_random.h: every word
// is jxs_rand::row_value of its row and its global environment).  One wave per tile, four tiles per workgroup, like
// jxs_env_select: the wave reads the T mask bytes of its tile first (one ballot; a null mask names every environment)
// and returns when none is set -- the sparse reset of a large batch costs the mask read only.  Otherwise, in its own
// slice of LDS ((12 + 2n + 10) * T words):
//   1. its lanes draw the 12 + 2n variables of the T environments, one Philox block each (jxs_rand::variable);
//   2. 10 T lanes compute the rows that are no variable -- quaternion, converted base velocity -- from them
//      (jxs_rand::derived_value: the sines and cosines run once per environment, not once per word);
//   3. its lanes run over the contiguous rows * T words of the tile in accesses of A bytes (the widest the tile span and
//      the block address allow, jxs_env::access_bytes), each word placed by jxs_rand::row_source: an access none of whose
//      columns is named is skipped, one all of whose columns are named is stored without a load, a mixed one is loaded,
//      patched and stored.  Padding columns are never named.
// The three steps of one wave follow each other in program order and LDS serves a wave's accesses in order; the fences
// keep the compiler from moving them.  No workgroup barrier: the waves of a workgroup share nothing and may have left.
// `tile` divides 64 (the host checks), so the column and the row of a word are a mask and a shift.
template <typename T, int A>
__global__ void __launch_bounds__(256) jxs_env_randomize_kernel(const uint8_t* mask, unsigned char* state, int rows, int N, int tile_shift,
                                                                long long tiles, jxs_rand::Shape shape, const T* bounds, uint64_t seed,
                                                                uint64_t draw, long long first_env) {
  constexpr int WB = sizeof(T), WPA = A / WB;  // bytes per word, words per access
  extern __shared__ __align__(16) unsigned char jxs_randomize_lds[];
  const int tile = 1 << tile_shift;
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tiles) return;  // (wave-uniform)
  const long long env = jxs_env::env_of(t, lane, tile);
  const unsigned long long bits = __ballot(lane < tile && !jxs_env::is_padding(env, N) && (mask == nullptr || mask[env] != 0));
  if (bits == 0) return;  // (wave-uniform)
  const int nv = jxs_rand::n_variables(shape.n_joints);
  T* vars = reinterpret_cast<T*>(jxs_randomize_lds) + (size_t)(threadIdx.x >> 6) * (size_t)((nv + jxs_rand::kDerived) << tile_shift);
  T* derived = vars + ((size_t)nv << tile_shift);  // [kDerived][T] behind [nv][T]
  const uint32_t env0 = (uint32_t)(first_env + t * tile);  // (the host checked that every named environment fits 32 bits)
  for (int i = lane; i < (nv << tile_shift); i += 64) {
    const int col = i & (tile - 1);
    if ((bits >> col) & 1ull) vars[i] = jxs_rand::variable(bounds, nv, i >> tile_shift, seed, draw, env0 + (uint32_t)col);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int i = lane; i < (jxs_rand::kDerived << tile_shift); i += 64) {
    const int col = i & (tile - 1), d = i >> tile_shift;
    // (a value no row takes -- the velocity of a fixed base, of the Inertial representation -- is not computed)
    const bool used = d < 4 || (shape.floating && (shape.repr == jxs_rand::kReprBody || (shape.repr == jxs_rand::kReprMixed && d < 7)));
    if (used && ((bits >> col) & 1ull)) derived[i] = jxs_rand::derived_value<T>(shape, d, [&](int v) { return vars[(v << tile_shift) + col]; });
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int per_tile = (int)jxs_env::tile_words(rows, tile);  // (the host refuses a tile of 2^30 words)
  const int n_acc = per_tile / WPA;                            // (the host chose A so that this is exact)
  unsigned char* tp = state + (size_t)t * (size_t)per_tile * WB;
  for (int i = lane; i < n_acc; i += 64) {
    bool take[WPA], some = false, all = true;
#pragma unroll
    for (int j = 0; j < WPA; ++j) {
      take[j] = ((bits >> ((i * WPA + j) & (tile - 1))) & 1ull) != 0;
      some = some || take[j];
      all = all && take[j];
    }
    if (!some) continue;
    EnvPack<A>* p = reinterpret_cast<EnvPack<A>*>(tp + (size_t)i * A);
    EnvPack<A> v;
    if (!all) v = *p;
#pragma unroll
    for (int j = 0; j < WPA; ++j) {
      if (!take[j]) continue;
      const int w = i * WPA + j, col = w & (tile - 1);
      const jxs_rand::RowSource src = jxs_rand::row_source(shape, w >> tile_shift);
      T x = T(0);
      if (src.kind == jxs_rand::kRowVariable) x = vars[(src.index << tile_shift) + col];
      else if (src.kind == jxs_rand::kRowDerived) x = derived[(src.index << tile_shift) + col];
      __builtin_memcpy(&v.u[j * (WB / 4)], &x, WB);
    }
    *p = v;
  }
}

// The observation tensor out[N][out_ld] of a policy (the slots are jxs_env_observe.h: every word is jxs_obs::slot_value of
// its slot and its environment).  A wave takes E = 2^env_shift consecutive environments -- whole tiles, E >= T --, four
// waves per workgroup that share nothing:
//   1. its lanes compute the unit quaternion of the E environments, 4 E values (jxs_obs::unit_quaternion_component), and
//   2. from those the other derived values a slot of the table reads, up to 18 E (jxs_obs::derived_from_unit), into the
//      wave's slice of LDS, [kDerived][E]: the square root, the divisions and the rotations run once per environment, not
//      once per word.  A table without derived slots skips both steps and uses no LDS word;
//   3. lane c takes the columns c, c + 64, ... of the tensor: it reads the slot, offset and scale of a column ONCE, into
//      registers, and runs over the E environments: the word of a state or source row comes from global memory (lanes of
//      neighbouring rows read neighbouring words of a tile, T words apart), a derived one from LDS, and the 64 lanes store
//      64 consecutive words of the environment's row of `out`.
// The table is thus read once per wave whatever D is (no LDS copy that would bound D), and the stores of a row are
// contiguous; the lanes at and beyond D of the last 64 columns idle.  Only environments below N are touched: the padding
// columns of the last tile are neither read nor turned into rows, and a source is read at rows below its own count only
// (the host checked every slot), at the tile and column of an environment below N.  The steps of one wave follow each
// other in program order and LDS serves a wave's accesses in order; the fences keep the compiler from moving them.
struct ObsSources {
  const void* ptr[jxs_obs::kSources];
  int rows[jxs_obs::kSources];
};

// Steps 1 and 2 of jxs_env_observe_kernel and of jxs_env_evaluate_kernel: the derived values `used` names, of the wave's
// n_env environments, into its LDS slice derived[kDerived][E].  word_at(rows, row, e) is the word of a row of environment e
// of the wave in a tiled block of `rows` rows.  Ends behind the wave's barrier: every lane may read every value.
template <typename T, typename WordAt>
__device__ __forceinline__ void env_derived_values(const T* __restrict__ state, const jxs_obs::Shape& sh, unsigned used, int lane, int env_shift,
                                                   int n_env, T* derived, WordAt word_at) {
  const int E = 1 << env_shift;
  for (int i = lane; i < (jxs_obs::kDerivedRot << env_shift); i += 64) {
    const int e = i & (E - 1), k = i >> env_shift;
    if (((used >> k) & 1u) && e < n_env) {
      T q[4];
      for (int j = 0; j < 4; ++j) q[j] = state[word_at(sh.n_rows, jxs_obs::row_quat(sh) + j, e)];
      derived[i] = jxs_obs::unit_quaternion_component(q, k);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int i = (jxs_obs::kDerivedRot << env_shift) + lane; i < (jxs_obs::kDerived << env_shift); i += 64) {
    const int e = i & (E - 1), d = i >> env_shift;
    if (((used >> d) & 1u) && e < n_env) {
      T u[4];
      for (int j = 0; j < 4; ++j) u[j] = (used & 1u) ? derived[(j << env_shift) + e] : T(0);
      derived[i] = jxs_obs::derived_from_unit<T>(sh, d, u, [&](int r) { return state[word_at(sh.n_rows, r, e)]; });
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, typename O>
__global__ void __launch_bounds__(256) jxs_env_observe_kernel(const T* __restrict__ state, ObsSources src, const int32_t* __restrict__ codes,
                                                              const T* __restrict__ offset, const T* __restrict__ scale, int D, unsigned used,
                                                              jxs_obs::Shape sh, int N, int tile_shift, int env_shift, O* __restrict__ out,
                                                              long long out_ld) {
  extern __shared__ __align__(16) unsigned char jxs_observe_lds[];
  const int lane = threadIdx.x & 63;
  const int E = 1 << env_shift, tmask = (1 << tile_shift) - 1;
  const long long env0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) << env_shift;
  if (env0 >= N) return;  // (wave-uniform)
  const int n_env = (long long)N - env0 < E ? (int)(N - env0) : E;
  T* derived = reinterpret_cast<T*>(jxs_observe_lds) + (size_t)(threadIdx.x >> 6) * (size_t)(jxs_obs::kDerived << env_shift);
  // word of row `row` of environment env0 + e in a tiled block of `rows` rows (rows * T < 2^30: the host checks)
  auto word_at = [&](int rows, int row, int e) {
    const long long env = env0 + e;
    return (size_t)(env >> tile_shift) * (size_t)(rows << tile_shift) + (size_t)((row << tile_shift) + (int)(env & tmask));
  };
  // (the slot of the lane's first column is asked for now: its three loads travel with those of the derived values
  // instead of starting a further round trip behind them)
  int32_t code = 0;
  T off = T(0), sc = T(1);
  if (lane < D) code = codes[lane], off = offset[lane], sc = scale[lane];
  if (used != 0) env_derived_values(state, sh, used, lane, env_shift, n_env, derived, word_at);
  O* const orow = out + (size_t)env0 * (size_t)out_ld;
  for (int c = lane; c < D; c += 64) {
    if (c != lane) code = codes[c], off = offset[c], sc = scale[c];
    const int kind = jxs_obs::packed_kind(code), index = jxs_obs::packed_index(code), s = jxs_obs::packed_source(code);
    const bool from_row = kind <= jxs_obs::kSourceRow, from_source = kind == jxs_obs::kSourceRow;
    const T* base = !from_source ? state : static_cast<const T*>(s == 0 ? src.ptr[0] : s == 1 ? src.ptr[1] : s == 2 ? src.ptr[2] : src.ptr[3]);
    const int rows = !from_source ? sh.n_rows : (s == 0 ? src.rows[0] : s == 1 ? src.rows[1] : s == 2 ? src.rows[2] : src.rows[3]);
#pragma unroll 4
    for (int e = 0; e < n_env; ++e) {
      const T x = from_row ? base[word_at(rows, index, e)] : derived[(index << env_shift) + e];  // (one load per lane, by its kind)
      orow[(size_t)e * (size_t)out_ld + c] = (O)jxs_obs::affine(x, off, sc);
    }
  }
}

// The reward, the done byte and their optional companions of every environment (the law is jxs_env_evaluate.h: every output
// is what jxs_eval::evaluate_env gives for its environment).  The frame of jxs_env_observe_kernel: a wave takes E =
// 2^env_shift consecutive environments -- whole tiles, E >= T --, and the waves of a workgroup (4, or 2 or 1 where the LDS
// of 4 would pass 64 KB) share nothing.  A wave's LDS slice is [kDerived + K + C][E] words:
//   1., 2. the derived values the table's slots read (env_derived_values, as in the observation), skipped without such slots;
//   3. work items i = lane, lane + 64, ... over (K + C) x E, environment fastest, so that the lanes of one term read
//      neighbouring columns of a tile.  A term item walks its slots in order -- the slot words are uniform across the lanes
//      of a term, x comes from global memory or from the derived slice --, accumulates, applies outer, weight and clamp, and
//      stores p into LDS [K][E] (and into `terms`); a condition item stores whether it fired into LDS [C][E];
//   4. lane e < n_env sums the p of its environment in term order, ORs the bits, applies the counter rule and stores
//      reward, done, fired and steps: the stores of the lanes are contiguous.
// Only environments below N are touched: padding columns of the last tile are never read, a source is read at rows below
// its own count only (the host checked every slot and target).  The steps of one wave follow each other in program order and
// LDS serves a wave's accesses in order; the fences keep the compiler from moving them.
template <typename T>
struct EvalTable {
  const int32_t* codes;     // [D]
  const int32_t* targets;   // [D]
  const T* offset;          // [D]
  const T* scale;           // [D]
  const int32_t* terms;     // [K][4]
  const T* term_params;     // [K][3]
  const int32_t* conds;     // [C][2]
  const T* cond_limits;     // [C][2]
  int K, C;
  T reward_lo, reward_hi, termination_reward;
};

template <typename T, typename R, typename TT>
__global__ void __launch_bounds__(256) jxs_env_evaluate_kernel(const T* __restrict__ state, ObsSources src, EvalTable<T> tb, unsigned used,
                                                               jxs_obs::Shape sh, int N, int tile_shift, int env_shift, R* __restrict__ reward,
                                                               uint8_t* __restrict__ done, uint32_t* __restrict__ fired, TT* __restrict__ terms,
                                                               long long terms_ld, int32_t* __restrict__ steps, int max_steps) {
  extern __shared__ __align__(16) unsigned char jxs_evaluate_lds[];
  const int lane = threadIdx.x & 63;
  const int E = 1 << env_shift, tmask = (1 << tile_shift) - 1;
  const int K = tb.K, C = tb.C;
  const long long env0 = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) << env_shift;
  if (env0 >= N) return;  // (wave-uniform)
  const int n_env = (long long)N - env0 < E ? (int)(N - env0) : E;
  T* derived = reinterpret_cast<T*>(jxs_evaluate_lds) + (size_t)(threadIdx.x >> 6) * (size_t)((jxs_obs::kDerived + K + C) << env_shift);
  T* const contrib = derived + (jxs_obs::kDerived << env_shift);                          // [K][E]
  uint32_t* const fire = reinterpret_cast<uint32_t*>(contrib + ((size_t)K << env_shift));  // [C][E], one word of T each
  // word of row `row` of environment env0 + e in a tiled block of `rows` rows (rows * T < 2^30: the host checks)
  auto word_at = [&](int rows, int row, int e) {
    const long long env = env0 + e;
    return (size_t)(env >> tile_shift) * (size_t)(rows << tile_shift) + (size_t)((row << tile_shift) + (int)(env & tmask));
  };
  auto source = [&](int s) { return static_cast<const T*>(s == 0 ? src.ptr[0] : s == 1 ? src.ptr[1] : s == 2 ? src.ptr[2] : src.ptr[3]); };
  auto source_rows = [&](int s) { return s == 0 ? src.rows[0] : s == 1 ? src.rows[1] : s == 2 ? src.rows[2] : src.rows[3]; };
  if (used != 0) env_derived_values(state, sh, used, lane, env_shift, n_env, derived, word_at);
  const bool want_terms = reward != nullptr || terms != nullptr;  // (without either nobody reads a contribution)
  for (int i = lane; i < ((K + C) << env_shift); i += 64) {
    const int e = i & (E - 1), item = i >> env_shift;
    if (e >= n_env || (item < K && !want_terms)) continue;
    // (A term item walks its slots one at a time.  Asking for the loads of eight slots at once, unconditionally, measured
    // slower, not faster -- profiles/env_evaluate_chunked_loads.txt against profiles/env_evaluate.txt --: the walk is bound by
    // the cache lines its accesses touch, not by their latency)
    auto y = [&](int d) {
      const int32_t code = tb.codes[d], tg = tb.targets[d];
      const int kind = jxs_obs::packed_kind(code), index = jxs_obs::packed_index(code), s = jxs_obs::packed_source(code);
      T raw;
      if (kind == jxs_obs::kStateRow) raw = state[word_at(sh.n_rows, index, e)];
      else if (kind == jxs_obs::kSourceRow) raw = source(s)[word_at(source_rows(s), index, e)];
      else raw = derived[(index << env_shift) + e];
      T target = T(0);
      if (tg >= 0) target = source(jxs_eval::target_source(tg))[word_at(source_rows(jxs_eval::target_source(tg)), jxs_eval::target_row(tg), e)];
      return jxs_obs::affine(jxs_eval::slot_x(raw, tg >= 0, target), tb.offset[d], tb.scale[d]);
    };
    if (item < K) {
      const int32_t* info = tb.terms + 4 * item;
      const T* w = tb.term_params + 3 * item;
      const T p = jxs_eval::term_value<T>(info[0], info[1], info[2], info[3], w[0], w[1], w[2], y);
      contrib[i] = p;
      if (terms != nullptr) terms[(size_t)(env0 + e) * (size_t)terms_ld + item] = (TT)p;
    } else {
      const int c = item - K;
      fire[(c << env_shift) + e] = jxs_eval::fires(y(tb.conds[2 * c]), tb.cond_limits[2 * c], tb.cond_limits[2 * c + 1]) ? 1u : 0u;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < n_env) {
    const size_t env = (size_t)env0 + lane;
    unsigned dn = 0, fr = 0;
    for (int c = 0; c < C; ++c)
      if (fire[(c << env_shift) + lane] != 0) fr |= 1u << c, dn |= 1u << tb.conds[2 * c + 1];
    if (steps != nullptr) steps[env] = jxs_eval::counted(steps[env], max_steps, &dn);
    if (reward != nullptr) {
      const T r = jxs_eval::total<T>(K, tb.reward_lo, tb.reward_hi, [&](int t) { return contrib[(t << env_shift) + lane]; });
      reward[env] = (R)jxs_eval::terminal(r, dn, tb.termination_reward);
    }
    if (done != nullptr) done[env] = (uint8_t)dn;
    if (fired != nullptr) fired[env] = fr;
  }
}

// The joint torques out[n][N] (tiled) of a policy's action tensor actions[N][act_ld] (the arithmetic is jxs_env_act.h:
// every word is jxs_act::torque_word of its joint and its environment).  A wave takes E = 2^env_shift consecutive
// environments -- whole tiles, E >= T --, four waves per workgroup that share nothing.  Its lanes run over the words of its
// tiles of `out` in accesses of AB bytes (the widest the tile spans and the block addresses allow, jxs_env::access_bytes).
// Word w = j T + c of a tile belongs to joint j and column c, and the q rows (state rows 7 ..), the qd rows (13 + n ..),
// feed_forward and out are each one contiguous span of n T words per tile, so the same access index serves all four.  The
// action tensor is the one transposed operand: a lane gathers actions[e][column_j], so neighbouring lanes read words act_ld
// apart -- but the E rows of a wave are one short stretch of memory whose lines the wave uses whole, and staging them
// through LDS first measured slower (profiles/env_act_both_reads.txt).  The joint's packed word and
// its eight parameters are read by joint index; the T lanes of a joint read the same record.
// Only action rows below N are read.  The padding columns of the last tile are read from the state and from feed_forward
// with the access they share with real columns, never used, and written as zero.
template <typename T, typename AT, int AB>
__global__ void __launch_bounds__(256) jxs_env_act_kernel(const T* __restrict__ state, const AT* __restrict__ actions, long long act_ld,
                                                          const int32_t* __restrict__ codes, const jxs_act::Params<T>* __restrict__ params,
                                                          const T* __restrict__ ff, T* __restrict__ out, int n, int n_rows, int N,
                                                          int tile_shift, int env_shift) {
  constexpr int WB = sizeof(T), WPA = AB / WB;  // bytes per word, words per access
  const int lane = threadIdx.x & 63;
  const int E = 1 << env_shift, tile = 1 << tile_shift, tmask = tile - 1;
  const long long env0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) << env_shift;
  if (env0 >= N) return;  // (wave-uniform)
  const int n_env = (long long)N - env0 < E ? (int)(N - env0) : E;
  const int n_tiles = (n_env + tmask) >> tile_shift;
  const AT* const arow = actions == nullptr ? nullptr : actions + (size_t)env0 * (size_t)act_ld;
  const int span = n << tile_shift;  // words of the joints of one tile (n * T < 2^30: the host checks)
  const unsigned per_tile = (unsigned)(span / WPA);  // (the host chose AB so that this is exact)
  const size_t tile0 = (size_t)(env0 >> tile_shift);
  const unsigned char* const qp = reinterpret_cast<const unsigned char*>(state + tile0 * ((size_t)n_rows << tile_shift) + ((size_t)jxs_act::row_q(n) << tile_shift));
  const size_t qd_at = (size_t)((jxs_act::row_qd(n) - jxs_act::row_q(n)) << tile_shift) * WB;  // bytes from a tile's q rows to its qd rows
  const size_t state_tile = ((size_t)n_rows << tile_shift) * WB;
  const unsigned char* const fp = ff == nullptr ? nullptr : reinterpret_cast<const unsigned char*>(ff + tile0 * (size_t)span);
  unsigned char* const op = reinterpret_cast<unsigned char*>(out + tile0 * (size_t)span);
  for (unsigned i = lane; i < (unsigned)n_tiles * per_tile; i += 64) {
    const unsigned tl = i / per_tile, r = i - tl * per_tile;  // tile of the wave, access inside the tile's span
    const unsigned char* const qa = qp + (size_t)tl * state_tile + (size_t)r * AB;
    const EnvPack<AB> vq = *reinterpret_cast<const EnvPack<AB>*>(qa);
    const EnvPack<AB> vqd = *reinterpret_cast<const EnvPack<AB>*>(qa + qd_at);
    EnvPack<AB> vff{}, v;
    if (fp != nullptr) vff = *reinterpret_cast<const EnvPack<AB>*>(fp + (size_t)i * AB);
#pragma unroll
    for (int k = 0; k < WPA; ++k) {
      const int w = (int)r * WPA + k, j = w >> tile_shift;
      const int e = (int)(tl << tile_shift) + (w & tmask);
      T t = T(0);
      if (e < n_env) {
        const int32_t code = codes[j];
        const jxs_act::Params<T> p = params[j];
        const int column = jxs_act::packed_column(code);
        T a = T(0);
        if (column >= 0) a = (T)arow[(size_t)e * (size_t)act_ld + column];
        T q, qd, f = T(0);
        __builtin_memcpy(&q, &vq.u[k * (WB / 4)], WB);
        __builtin_memcpy(&qd, &vqd.u[k * (WB / 4)], WB);
        if (fp != nullptr) __builtin_memcpy(&f, &vff.u[k * (WB / 4)], WB);
        t = jxs_act::torque_word(jxs_act::packed_mode(code), column, a, p.v, q, qd, fp != nullptr, f);
      }
      __builtin_memcpy(&v.u[k * (WB / 4)], &t, WB);
    }
    *reinterpret_cast<EnvPack<AB>*>(op + (size_t)i * AB) = v;
  }
}

// The contact record out[G * 8][N] (tiled) and the timers [G * 2][N] (tiled, in/out) of every environment from its link
// transforms and velocities (the law is jxs_env_contact.h: every word is what jxs_contact::sense_env gives for its
// environment).  The frame of jxs_env_observe_kernel: a wave takes E = 2^env_shift consecutive environments -- whole tiles,
// E >= T --, and the waves of a workgroup (4, or 2 or 1 where the LDS of 4 would pass 64 KB) share nothing.  The points of an
// environment are independent, so they get lanes; the entries of the table are taken in chunks of `chunk` points
// (chunk * E <= 512 items, all of them for the tables of a legged robot):
//   1. work items i = lane, lane + 64, ... over chunk x E, environment fastest, so that the lanes of a point read neighbouring
//      columns of a tile.  An item reads the 12 transform and 6 velocity rows of its point's parent link -- 18 independent
//      loads --, evaluates jxs_contact::point_sample and stores clearance and slip into the wave's LDS [2][chunk * E];
//   2. work items j over G x E, environment fastest: an item folds the samples of its group that lie in this chunk, from
//      LDS, in entry order (jxs_contact::fold: the sequential rule of the law, which a NaN and a signed zero make
//      order-dependent).  A group that ends in this chunk applies the timer rule (jxs_contact::finish) and stores its 8 record
//      rows and 2 timer rows: the stores of the lanes of a row are contiguous.  A group that goes on keeps its fold in LDS
//      [3][G * E].
// Last, the padding columns of the last tile of the record are written as zero.  Only environments below N are read: no
// padding column of a block, and no byte of the mask beyond N.  The steps of one wave follow each other in program order and
// LDS serves a wave's accesses in order; the fences keep the compiler from moving them.
template <typename T>
struct ContactTable {
  const int32_t* groups;  // [G][2]
  const int32_t* parent;  // [P]
  const T* L_p;           // [P][3]
  int G, P;
};

template <typename T>
__global__ void __launch_bounds__(256) jxs_env_contacts_kernel(const T* __restrict__ link_H, const T* __restrict__ link_V, ContactTable<T> tb,
                                                               jxs_contact::Terrain<T> tr, int n_links, int N, int tile_shift, int env_shift, int chunk,
                                                               T dt, const uint8_t* __restrict__ reset_mask, T* __restrict__ timers,
                                                               T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char jxs_contacts_lds[];
  const int lane = threadIdx.x & 63;
  const int E = 1 << env_shift, tile = 1 << tile_shift, tmask = tile - 1;
  const int G = tb.G, P = tb.P;
  const long long env0 = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) << env_shift;
  if (env0 >= N) return;  // (wave-uniform)
  const int n_env = (long long)N - env0 < E ? (int)(N - env0) : E;
  const int items = chunk << env_shift;
  T* const clearance = reinterpret_cast<T*>(jxs_contacts_lds) + (size_t)(threadIdx.x >> 6) * (size_t)(2 * items + ((3 * G) << env_shift));
  T* const slip = clearance + items;
  T* const kept = slip + items;  // [3][G * E]: count, clearance, slip of a group that spans chunks
  // word of row `row` of environment env0 + e in a tiled block of `rows` rows (rows * T < 2^30: the host checks)
  auto word_at = [&](int rows, int row, int e) {
    const long long env = env0 + e;
    return (size_t)(env >> tile_shift) * (size_t)(rows << tile_shift) + (size_t)((row << tile_shift) + (int)(env & tmask));
  };
  const int rows_H = 12 * n_links, rows_V = 6 * n_links, rows_out = jxs_contact::kRows * G, rows_t = jxs_contact::kTimerRows * G;
  for (int k0 = 0; k0 < P; k0 += chunk) {
    const int k1 = k0 + chunk < P ? k0 + chunk : P;
    for (int i = lane; i < ((k1 - k0) << env_shift); i += 64) {
      const int e = i & (E - 1), k = k0 + (i >> env_shift);
      if (e >= n_env) continue;
      const int l = tb.parent[k];
      const T L_p[3] = {tb.L_p[3 * k], tb.L_p[3 * k + 1], tb.L_p[3 * k + 2]};
      const size_t at_H = word_at(rows_H, 12 * l, e);
      T h[12], v[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int r = 0; r < 12; ++r) h[r] = link_H[at_H + ((size_t)r << tile_shift)];
      if (link_V != nullptr) {
        const size_t at_V = word_at(rows_V, 6 * l, e);
#pragma unroll
        for (int r = 0; r < 6; ++r) v[r] = link_V[at_V + ((size_t)r << tile_shift)];
      }
      const jxs_contact::Sample<T> s = jxs_contact::point_sample(tr, L_p, link_V != nullptr, [&](int r) { return h[r]; }, [&](int r) { return v[r]; });
      clearance[i] = s.clearance, slip[i] = s.slip_sq;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int j = lane; j < (G << env_shift); j += 64) {
      const int e = j & (E - 1), g = j >> env_shift;
      if (e >= n_env) continue;
      const int first = tb.groups[2 * g], end = first + tb.groups[2 * g + 1];
      const int lo = first > k0 ? first : k0, hi = end < k1 ? end : k1;
      if (lo >= hi) continue;
      jxs_contact::Fold<T> f{T(0), T(0), T(0)};
      if (lo != first) f = jxs_contact::Fold<T>{kept[j], kept[(G << env_shift) + j], kept[((2 * G) << env_shift) + j]};
      for (int k = lo; k < hi; ++k) {
        const int i = ((k - k0) << env_shift) + e;
        f = jxs_contact::fold(k == first, f, jxs_contact::Sample<T>{clearance[i], slip[i]});
      }
      if (hi != end) {
        kept[j] = f.count, kept[(G << env_shift) + j] = f.clearance, kept[((2 * G) << env_shift) + j] = f.slip_sq;
        continue;
      }
      T a = T(0), b = T(0), rec[jxs_contact::kRows];
      const size_t at_t = timers != nullptr ? word_at(rows_t, jxs_contact::kTimerRows * g, e) : 0;
      if (timers != nullptr) a = timers[at_t], b = timers[at_t + tile];
      const bool reset = reset_mask != nullptr && reset_mask[env0 + e] != 0;
      jxs_contact::finish(f, timers != nullptr, reset, dt, &a, &b, rec);
      if (timers != nullptr) timers[at_t] = a, timers[at_t + tile] = b;
      const size_t at_o = word_at(rows_out, jxs_contact::kRows * g, e);
#pragma unroll
      for (int r = 0; r < jxs_contact::kRows; ++r) out[at_o + ((size_t)r << tile_shift)] = rec[r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // the padding columns of the last tile: env0 + e in [N, whole tiles)
  const int n_cols = ((n_env + tmask) >> tile_shift) << tile_shift;
  if (n_cols > n_env)
    for (int j = lane; j < (rows_out << env_shift); j += 64) {
      const int e = j & (E - 1), row = j >> env_shift;
      if (e >= n_env && e < n_cols) out[word_at(rows_out, row, e)] = T(0);
    }
}

namespace {
// ---- the host side of the per-environment operations: what their entry points share.  Every refusal comes before the launch and names its entry point (`who`).

int refuse(const char* who, const std::string& what) { return fail(JXS_EINVAL, std::string(who) + ": " + what); }

bool repr_ok(int r) { return r == JXS_REPR_INERTIAL || r == JXS_REPR_BODY || r == JXS_REPR_MIXED; }

// The env kernels' view of a model: a tile of T = 64 / G = 2^tile_shift environments, whole tiles per wave, and the words
// of a tile of `rows` rows (the state's, or the tallest block the launch reads) counted in 32 bits with room to spare.
struct EnvTile {
  int tile = 0, tile_shift = 0;
};
int env_tile(const char* who, int G, int rows, EnvTile& t) {
  t.tile = G > 0 ? 64 / G : 0, t.tile_shift = 0;
  while ((1 << t.tile_shift) < t.tile) ++t.tile_shift;
  if (t.tile <= 0 || (1 << t.tile_shift) != t.tile || t.tile > 64) return refuse(who, "the model's tile does not divide the wave");
  if (jxs_env::tile_words(rows, t.tile) >= (1LL << 30)) return refuse(who, "rows * tile must be below 2^30");
  return JXS_OK;
}

// f(std::integral_constant<int, A>) for the access width A = `access` out of {16, 8, 4} bytes (jxs_env::access_bytes, never
// below the word): the kernels take it at compile time, and words of WB = 8 bytes have no 4-byte variant.
template <int WB, typename F>
void with_access(int access, F&& f) {
  if (access == 16) f(std::integral_constant<int, 16>{});
  else if (access == 8) f(std::integral_constant<int, 8>{});
  else if constexpr (WB == 4) f(std::integral_constant<int, 4>{});
}
// f(T{}) or f(float{}): the element type of the tensor a policy shares with the library, the model's own or float32
template <typename T, typename F>
void with_io_type(bool models_own, F&& f) {
  if (models_own) f(T{});
  else f(float{});
}

// the env kernels run four waves per workgroup, which share nothing
constexpr int kEnvBlock = 256;
dim3 env_grid(long long waves) { return dim3((unsigned)((waves + 3) / 4)); }
long long env_waves(int N, int env_shift) { return ((long long)N + (1LL << env_shift) - 1) >> env_shift; }
// ... except where a wave's LDS grows with its table: as many waves per workgroup, out of 4, 2, 1, as fit 64 KB, and the
// grid of such workgroups (env_grid counts four waves per workgroup: a workgroup of 4 / f waves needs f times as many)
int waves_that_fit(size_t per_wave_bytes) {
  int waves_per_block = 4;
  while (waves_per_block > 1 && waves_per_block * per_wave_bytes > 64 * 1024) waves_per_block >>= 1;
  return waves_per_block;
}
dim3 env_grid(long long waves, int waves_per_block) { return env_grid(waves * (4 / waves_per_block)); }

// The sources a launch reads, bound to the kernel's argument: those the table uses, refused when the pointer of one is null.
// Then, for the caller's tile and alignment checks: the rows of the tallest, and the OR of their addresses.
int bind_sources(const char* who, unsigned used, const int32_t* table_rows, const void* const sources[4], ObsSources& src) {
  for (int s = 0; s < jxs_obs::kSources; ++s) {
    if (!((used >> s) & 1u)) continue;  // (a pointer the table does not use is not looked at)
    if (sources == nullptr || sources[s] == nullptr) return refuse(who, "the table reads source " + std::to_string(s) + ", whose pointer is null");
    src.ptr[s] = sources[s], src.rows[s] = table_rows[s];
  }
  return JXS_OK;
}
int max_rows(const ObsSources& src) { return *std::max_element(src.rows, src.rows + jxs_obs::kSources); }
uintptr_t addresses(const ObsSources& src) { return (uintptr_t)src.ptr[0] | (uintptr_t)src.ptr[1] | (uintptr_t)src.ptr[2] | (uintptr_t)src.ptr[3]; }

// after the launch: what the runtime says about it
int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, who) : (int)JXS_OK;
}

// was this table (jxs_observation, jxs_action) created for the state layout and dtype of this model?
template <typename Table, typename KP>
bool table_fits(const Table& t, int dtype, const KP& P) {
  return t.dtype == dtype && t.n_rows == P.n_rows && t.n_joints == P.n;
}

// what every *_create checks first: a place for the table, cleared, and a model
template <typename Table>
int create_preamble(const jxs_model* model, Table** out) {
  if (out == nullptr) return fail(JXS_EINVAL, "null out");
  *out = nullptr;
  return model == nullptr ? fail(JXS_EINVAL, "null model") : (int)JXS_OK;
}

// A host table on the device (blocking; the tables are a few KB) and its object in *out, or the error set and *out left null;
// and the end of a table object.  hipFree waits for the launches that may still read the table.
template <typename Table>
int upload_table(std::unique_ptr<Table> t, const std::vector<unsigned char>& host, const char* what, Table** out) {
  hipError_t e = hipMalloc(&t->table, host.size());
  if (e == hipSuccess && (e = hipMemcpy(t->table, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess) (void)hipFree(t->table);
  if (e != hipSuccess) return hip_fail(e, what);
  *out = t.release();
  return JXS_OK;
}
template <typename Table>
int destroy_table(Table* t) {
  if (t != nullptr) (void)hipFree(t->table);
  delete t;
  return JXS_OK;
}
}  // namespace

extern "C" {

int jxs_env_select(const uint8_t* mask, const void* a, const void* b, void* out, int rows, int N, int tile, int dtype, void* stream) {
  if (mask == nullptr || a == nullptr || b == nullptr || out == nullptr) return fail(JXS_EINVAL, "null argument");
  if (rows <= 0 || N <= 0 || tile <= 0) return fail(JXS_EINVAL, "rows, N and tile must be positive");
  if (dtype != JXS_F32 && dtype != JXS_F64) return fail(JXS_EINVAL, "dtype must be JXS_F32 or JXS_F64");
  const int wb = dtype == JXS_F64 ? 8 : 4;
  const unsigned long long addr = (unsigned long long)(uintptr_t)a | (uintptr_t)b | (uintptr_t)out;
  if (addr % wb != 0) return fail(JXS_EINVAL, "a, b and out must be aligned to their element type");
  if (jxs_env::tile_words(rows, tile) >= (1LL << 30)) return fail(JXS_EINVAL, "rows * tile must be below 2^30");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long tiles = jxs_env::n_tiles(N, tile);
  auto launch = [&](auto word) {  // (the kernel moves words as bytes: it takes their size, not their type)
    constexpr int WB = decltype(word)::value;
    with_access<WB>(jxs_env::access_bytes(addr, rows, tile, WB), [&](auto ab) {
      hipLaunchKernelGGL((jxs_env_select_kernel<decltype(ab)::value, WB>), env_grid(tiles), dim3(kEnvBlock), 0, s, mask, (const unsigned char*)a,
                         (const unsigned char*)b, (unsigned char*)out, rows, N, tile, tiles);
    });
  };
  if (wb == 4) launch(std::integral_constant<int, 4>{});
  else launch(std::integral_constant<int, 8>{});
  return launched("jxs_env_select");
}

int jxs_env_copy(const void* src, int src_N, int src_tile, const int32_t* src_idx, void* dst, int dst_N, int dst_tile,
                 const int32_t* dst_idx, int rows, int K, int dtype, void* stream) {
  if (src == nullptr || dst == nullptr) return fail(JXS_EINVAL, "null argument");
  if (rows <= 0 || K <= 0 || src_N <= 0 || dst_N <= 0 || src_tile <= 0 || dst_tile <= 0)
    return fail(JXS_EINVAL, "rows, K, src_N, dst_N, src_tile and dst_tile must be positive");
  if (dtype != JXS_F32 && dtype != JXS_F64) return fail(JXS_EINVAL, "dtype must be JXS_F32 or JXS_F64");
  const long long total = (long long)K * rows;
  const int threads = 256;
  const long long blocks = (total + threads - 1) / threads;
  if (blocks > 0x7fffffffLL) return fail(JXS_EINVAL, "K * rows is too large for one launch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_dtype(dtype, [&](auto zero) {
    using W = std::conditional_t<sizeof(zero) == 8, uint64_t, uint32_t>;  // (words are moved as bits)
    hipLaunchKernelGGL(jxs_env_copy_kernel<W>, dim3((unsigned)blocks), dim3(threads), 0, s, (const W*)src, src_N, src_tile, src_idx, (W*)dst,
                       dst_N, dst_tile, dst_idx, rows, total);
  });
  return launched("jxs_env_copy");
}

int jxs_env_flags(jxs_model* model, const void* state, int N, uint8_t* out_flags, void* stream) {
  if (model == nullptr || state == nullptr || out_flags == nullptr) return fail(JXS_EINVAL, "null argument");
  if (N <= 0) return fail(JXS_EINVAL, "N must be positive");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    EnvTile t;
    if (const int rc = env_tile("jxs_env_flags", mt->pk.G, P.n_rows, t)) return rc;
    const long long tiles = jxs_env::n_tiles(N, t.tile);
    hipLaunchKernelGGL(jxs_env_flags_kernel<T>, env_grid(tiles), dim3(kEnvBlock), 0, s, static_cast<const T*>(state), P.n_rows, P.row_quat,
                       t.tile, N, tiles, out_flags);
    return launched("jxs_env_flags");
  });
}

int jxs_env_randomize(jxs_model* model, const uint8_t* mask, void* state, int N, const void* bounds, uint64_t seed, uint64_t draw,
                      int64_t first_env, int velocity_representation, void* stream) {
  if (model == nullptr || state == nullptr || bounds == nullptr) return fail(JXS_EINVAL, "null argument");
  if (N <= 0) return fail(JXS_EINVAL, "N must be positive");
  const char* const who = "jxs_env_randomize";
  if (!jxs_rand::env_range_ok(first_env, N)) return refuse(who, "first_env must be >= 0 and first_env + N <= 2^32");
  if (!repr_ok(velocity_representation)) return refuse(who, "unknown velocity representation");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    EnvTile t;
    if (const int rc = env_tile(who, mt->pk.G, P.n_rows, t)) return rc;
    const int tile = t.tile;
    if ((uintptr_t)state % sizeof(T) != 0 || (uintptr_t)bounds % sizeof(T) != 0) return refuse(who, "state and bounds must be aligned to their element type");
    const jxs_rand::Shape shape{P.n, P.floating, velocity_representation};
    // LDS of a workgroup: four waves, each the variables and the derived values of the T environments of its tile.
    // The packer gives an environment G >= max(4, pow2ceil(n_links)) lanes (jxs_pack.h), so T = 64 / G <= 16 and
    // n_joints < G: a wave needs at most (22 + 2 G) * 64 / G <= 480 words, a workgroup at most 15 KB in fp64.  The
    // refusal below cannot be reached with that rule; it is there so that a packer that ever allowed more (T = 64 with
    // many joints) fails here with a message instead of launching with more LDS than a workgroup may have -- the
    // remedy then is fewer waves per workgroup, not a larger limit.
    const size_t lds = 4 * (size_t)(jxs_rand::n_variables(P.n) + jxs_rand::kDerived) * tile * sizeof(T);
    if (lds > 65536) return refuse(who, "(12 + 2 n_joints + 10) * tile words per wave do not fit the LDS of a workgroup");
    const long long tiles = jxs_env::n_tiles(N, tile);
    with_access<sizeof(T)>(jxs_env::access_bytes((unsigned long long)(uintptr_t)state, P.n_rows, tile, (int)sizeof(T)), [&](auto ab) {
      hipLaunchKernelGGL((jxs_env_randomize_kernel<T, decltype(ab)::value>), env_grid(tiles), dim3(kEnvBlock), lds, s, mask,
                         static_cast<unsigned char*>(state), P.n_rows, N, t.tile_shift, tiles, shape, static_cast<const T*>(bounds), seed, draw,
                         (long long)first_env);
    });
    return launched(who);
  });
}

int jxs_observation_create(jxs_model* model, int D, const int32_t* slots, const double* offset, const double* scale,
                           const int32_t source_rows[4], jxs_observation** out) {
  if (const int rc = create_preamble(model, out)) return rc;
  if (slots == nullptr) return fail(JXS_EINVAL, "null slots");
  const char* const who = "jxs_observation_create";
  return with_typed(model, [&](auto* mt) -> int {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    int bad = -1;
    const int err = jxs_obs::table_error(slots, D, P.n_rows, source_rows, &bad);
    if (err == jxs_obs::kBadWidth)
      return refuse(who, "D = " + std::to_string(D) + " outside [1, " + std::to_string(JXS_OBS_MAX_WIDTH) + "]");
    if (err != jxs_obs::kOk) {
      const char* what = err == jxs_obs::kBadKind ? "unknown kind" : err == jxs_obs::kBadSource ? "source out of range or without rows" : "row or component out of range";
      return refuse(who, "slot " + std::to_string(bad) + " {" + std::to_string(slots[3 * bad]) + ", " + std::to_string(slots[3 * bad + 1]) + ", " +
                             std::to_string(slots[3 * bad + 2]) + "}: " + what);
    }
    auto ob = std::make_unique<jxs_observation>();
    ob->dtype = model->dtype, ob->D = D, ob->n_rows = P.n_rows, ob->n_joints = P.n;
    for (int s = 0; s < jxs_obs::kSources; ++s) {
      ob->source_rows[s] = source_rows != nullptr && source_rows[s] > 0 ? source_rows[s] : 0;
      if (ob->source_rows[s] >= (1 << 26)) return refuse(who, "a source of 2^26 rows or more");
    }
    if (P.n_rows >= (1 << 26)) return refuse(who, "a state of 2^26 rows or more");
    ob->offset_at = ((size_t)D * sizeof(int32_t) + 15) / 16 * 16;
    ob->scale_at = ob->offset_at + ((size_t)D * sizeof(T) + 15) / 16 * 16;
    std::vector<unsigned char> host(ob->scale_at + (size_t)D * sizeof(T), 0);
    int32_t* codes = reinterpret_cast<int32_t*>(host.data());
    T* off = reinterpret_cast<T*>(host.data() + ob->offset_at);
    T* sc = reinterpret_cast<T*>(host.data() + ob->scale_at);
    for (int d = 0; d < D; ++d) {
      const jxs_obs::Slot s{slots[3 * d], slots[3 * d + 1], slots[3 * d + 2]};
      const double o = offset != nullptr ? offset[d] : 0.0, c = scale != nullptr ? scale[d] : 1.0;
      if (!jxs_obs::affine_ok(o, T(0)) || !jxs_obs::affine_ok(c, T(0)))
        return refuse(who, "slot " + std::to_string(d) + ": offset or scale not finite in the model's dtype");
      codes[d] = jxs_obs::pack_slot(s), off[d] = static_cast<T>(o), sc[d] = static_cast<T>(c);
      if (s.kind == jxs_obs::kSourceRow) ob->sources_used |= 1u << s.source;
    }
    for (int r = 0; r < 3; ++r) ob->derived_used[r] = jxs_obs::derived_used(slots, D, r);
    return upload_table(std::move(ob), host, "uploading the observation table", out);
  });
}
int jxs_observation_destroy(jxs_observation* observation) { return destroy_table(observation); }

int jxs_env_observe(jxs_model* model, const jxs_observation* observation, const void* state, const void* const sources[4], int N,
                    int velocity_representation, void* out, int out_dtype, int64_t out_ld, void* stream) {
  const char* const who = "jxs_env_observe";
  if (model == nullptr || observation == nullptr || state == nullptr || out == nullptr) return refuse(who, "null argument");
  if (N <= 0) return refuse(who, "N must be positive");
  if (!repr_ok(velocity_representation)) return refuse(who, "unknown velocity representation");
  if (out_dtype != JXS_F32 && out_dtype != model->dtype) return refuse(who, "out_dtype must be JXS_F32 or the model's dtype");
  const jxs_observation& ob = *observation;
  if (out_ld < ob.D) return refuse(who, "out_ld = " + std::to_string(out_ld) + " below D = " + std::to_string(ob.D));
  ObsSources src{};
  if (const int rc = bind_sources(who, ob.sources_used, ob.source_rows, sources, src)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    if (!table_fits(ob, model->dtype, P)) return refuse(who, "the observation table was created for another state layout or dtype");
    EnvTile t;
    if (const int rc = env_tile(who, mt->pk.G, std::max(P.n_rows, max_rows(src)), t)) return rc;
    const size_t ob_bytes = out_dtype == JXS_F64 ? 8 : 4;
    if (((uintptr_t)state | addresses(src)) % sizeof(T) != 0 || (uintptr_t)out % ob_bytes != 0)
      return refuse(who, "state, sources and out must be aligned to their element type");
    const int env_shift = jxs_env::env_shift_for(N, t.tile_shift, knob(g_observe_envs_per_wave));
    const unsigned used = ob.derived_used[velocity_representation];
    const size_t lds = used != 0 ? 4 * (size_t)(jxs_obs::kDerived << env_shift) * sizeof(T) : 0;  // (at most 4 * 22 * 64 * 8 = 45 KB)
    const jxs_obs::Shape sh{P.n_rows, P.n, velocity_representation};
    const unsigned char* tb = static_cast<const unsigned char*>(ob.table);
    const int32_t* codes = reinterpret_cast<const int32_t*>(tb);
    const T* off = reinterpret_cast<const T*>(tb + ob.offset_at);
    const T* sc = reinterpret_cast<const T*>(tb + ob.scale_at);
    with_io_type<T>(out_dtype == model->dtype, [&](auto o) {
      using O = decltype(o);
      hipLaunchKernelGGL((jxs_env_observe_kernel<T, O>), env_grid(env_waves(N, env_shift)), dim3(kEnvBlock), lds, s, static_cast<const T*>(state),
                         src, codes, off, sc, ob.D, used, sh, N, t.tile_shift, env_shift, static_cast<O*>(out), (long long)out_ld);
    });
    return launched(who);
  });
}

int jxs_evaluation_create(jxs_model* model, const jxs_evaluation_desc* desc, jxs_evaluation** out) {
  if (const int rc = create_preamble(model, out)) return rc;
  if (desc == nullptr) return fail(JXS_EINVAL, "null desc");
  const char* const who = "jxs_evaluation_create";
  return with_typed(model, [&](auto* mt) -> int {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    const jxs_eval::Desc d{desc->D, desc->K, desc->C, desc->slots, desc->targets, desc->offset, desc->scale, desc->terms, desc->term_params,
                           desc->conditions, desc->condition_limits, desc->reward_lo, desc->reward_hi, desc->termination_reward};
    int bad = -1, slot_code = jxs_obs::kOk;
    const int err = jxs_eval::table_error(d, P.n_rows, desc->source_rows, T(0), &bad, &slot_code);
    if (err == jxs_eval::kBadWidth)
      return refuse(who, "D = " + std::to_string(desc->D) + ", K = " + std::to_string(desc->K) + ", C = " + std::to_string(desc->C) + " outside [1, " +
                             std::to_string(JXS_EVAL_MAX_SLOTS) + "], [0, " + std::to_string(JXS_EVAL_MAX_TERMS) + "], [0, " +
                             std::to_string(JXS_EVAL_MAX_CONDITIONS) + "], or a null table");
    if (err != jxs_eval::kOk) {
      const std::string at = std::to_string(bad);
      switch (err) {
        case jxs_eval::kBadSlot:
          return refuse(who, "slot " + at + ": " + (slot_code == jxs_obs::kBadKind ? "unknown kind" : slot_code == jxs_obs::kBadSource ? "source out of range or without rows" : "row or component out of range"));
        case jxs_eval::kBadTarget: return refuse(who, "slot " + at + ": target source or row out of range");
        case jxs_eval::kBadTerm: return refuse(who, "term " + at + ": unknown inner or outer");
        case jxs_eval::kBadRange: return refuse(who, "term " + at + ": an empty slot range, one outside the table or one that overlaps an earlier term's");
        case jxs_eval::kBadCondition: return refuse(who, "condition " + at + ": unknown kind, or a slot outside the table or owned already");
        case jxs_eval::kUnowned: return refuse(who, "slot " + at + " belongs to no term and no condition");
        case jxs_eval::kNotFinite:
          return refuse(who, (bad < 0 ? std::string("termination_reward") : "entry " + at + ": offset, scale or weight") + " not finite in the model's dtype");
        default: return refuse(who, (bad < 0 ? std::string("the reward limits") : "the limits of entry " + at) + ": lo above hi, NaN or not finite in the model's dtype");
      }
    }
    auto ev = std::make_unique<jxs_evaluation>();
    const int D = desc->D, K = desc->K, C = desc->C;
    ev->dtype = model->dtype, ev->D = D, ev->K = K, ev->C = C, ev->n_rows = P.n_rows, ev->n_joints = P.n;
    ev->reward_lo = desc->reward_lo, ev->reward_hi = desc->reward_hi, ev->termination_reward = desc->termination_reward;
    for (int s = 0; s < jxs_obs::kSources; ++s) {
      ev->source_rows[s] = desc->source_rows[s] > 0 ? desc->source_rows[s] : 0;
      if (ev->source_rows[s] >= (1 << 26)) return refuse(who, "a source of 2^26 rows or more");
    }
    if (P.n_rows >= (1 << 26)) return refuse(who, "a state of 2^26 rows or more");
    size_t at = 0;
    auto place = [&](size_t bytes) {
      const size_t here = at;
      at += (bytes + 15) / 16 * 16;
      return here;
    };
    place((size_t)D * sizeof(int32_t));
    ev->targets_at = place((size_t)D * sizeof(int32_t));
    ev->offset_at = place((size_t)D * sizeof(T));
    ev->scale_at = place((size_t)D * sizeof(T));
    ev->terms_at = place((size_t)K * 4 * sizeof(int32_t));
    ev->term_params_at = place((size_t)K * 3 * sizeof(T));
    ev->conds_at = place((size_t)C * 2 * sizeof(int32_t));
    ev->cond_limits_at = place((size_t)C * 2 * sizeof(T));
    std::vector<unsigned char> host(at + 16, 0);
    int32_t* codes = reinterpret_cast<int32_t*>(host.data());
    int32_t* targets = reinterpret_cast<int32_t*>(host.data() + ev->targets_at);
    T* off = reinterpret_cast<T*>(host.data() + ev->offset_at);
    T* sc = reinterpret_cast<T*>(host.data() + ev->scale_at);
    for (int i = 0; i < D; ++i) {
      const jxs_obs::Slot s{d.slots[3 * i], d.slots[3 * i + 1], d.slots[3 * i + 2]};
      const int ts = d.targets != nullptr ? d.targets[2 * i] : -1;
      codes[i] = jxs_obs::pack_slot(s), targets[i] = jxs_eval::pack_target(ts, ts < 0 ? 0 : d.targets[2 * i + 1]);
      off[i] = static_cast<T>(d.offset != nullptr ? d.offset[i] : 0.0), sc[i] = static_cast<T>(d.scale != nullptr ? d.scale[i] : 1.0);
      if (s.kind == jxs_obs::kSourceRow) ev->sources_used |= 1u << s.source;
      if (ts >= 0) ev->sources_used |= 1u << ts;
    }
    int32_t* terms = reinterpret_cast<int32_t*>(host.data() + ev->terms_at);
    T* tp = reinterpret_cast<T*>(host.data() + ev->term_params_at);
    for (int i = 0; i < 4 * K; ++i) terms[i] = d.terms[i];
    for (int i = 0; i < 3 * K; ++i) tp[i] = static_cast<T>(d.term_params[i]);
    int32_t* conds = reinterpret_cast<int32_t*>(host.data() + ev->conds_at);
    T* cl = reinterpret_cast<T*>(host.data() + ev->cond_limits_at);
    for (int i = 0; i < 2 * C; ++i) conds[i] = d.conds[i], cl[i] = static_cast<T>(d.cond_limits[i]);
    for (int r = 0; r < 3; ++r) ev->derived_used[r] = jxs_obs::derived_used(d.slots, D, r);
    return upload_table(std::move(ev), host, "uploading the evaluation table", out);
  });
}
int jxs_evaluation_destroy(jxs_evaluation* evaluation) { return destroy_table(evaluation); }

int jxs_env_evaluate(jxs_model* model, const jxs_evaluation* evaluation, const void* state, const void* const sources[4], int N,
                     int velocity_representation, void* reward, int reward_dtype, uint8_t* done, uint32_t* fired, void* terms, int terms_dtype,
                     int64_t terms_ld, int32_t* steps, int max_steps, void* stream) {
  const char* const who = "jxs_env_evaluate";
  if (model == nullptr || evaluation == nullptr || state == nullptr) return refuse(who, "null argument");
  if (reward == nullptr && done == nullptr) return refuse(who, "null reward and done: at least one of them is needed");
  if (N <= 0) return refuse(who, "N must be positive");
  if (!repr_ok(velocity_representation)) return refuse(who, "unknown velocity representation");
  if (reward != nullptr && reward_dtype != JXS_F32 && reward_dtype != model->dtype) return refuse(who, "reward_dtype must be JXS_F32 or the model's dtype");
  if (terms != nullptr && terms_dtype != JXS_F32 && terms_dtype != model->dtype) return refuse(who, "terms_dtype must be JXS_F32 or the model's dtype");
  const jxs_evaluation& ev = *evaluation;
  if (terms != nullptr && terms_ld < ev.K) return refuse(who, "terms_ld = " + std::to_string(terms_ld) + " below K = " + std::to_string(ev.K));
  if (steps != nullptr && max_steps <= 0) return refuse(who, "steps is given, and max_steps = " + std::to_string(max_steps) + " is not positive");
  ObsSources src{};
  if (const int rc = bind_sources(who, ev.sources_used, ev.source_rows, sources, src)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    if (!table_fits(ev, model->dtype, P)) return refuse(who, "the evaluation table was created for another state layout or dtype");
    EnvTile t;
    if (const int rc = env_tile(who, mt->pk.G, std::max(P.n_rows, max_rows(src)), t)) return rc;
    const bool own_reward = reward == nullptr || reward_dtype == model->dtype, own_terms = terms == nullptr || terms_dtype == model->dtype;
    const bool aligned = ((uintptr_t)state | addresses(src)) % sizeof(T) == 0 && (uintptr_t)reward % (own_reward ? sizeof(T) : 4) == 0 &&
                         (uintptr_t)terms % (own_terms ? sizeof(T) : 4) == 0 && (uintptr_t)fired % 4 == 0 && (uintptr_t)steps % 4 == 0;
    if (!aligned) return refuse(who, "state, sources, reward, terms, fired and steps must be aligned to their element type");
    const int env_shift = jxs_env::env_shift_for(N, t.tile_shift, knob(g_evaluate_envs_per_wave));
    // (kDerived + K + C) E words per wave (the worst case, 86 records of 64 fp64 environments, is 44 KB for one wave)
    const size_t per_wave = (size_t)((jxs_obs::kDerived + ev.K + ev.C) << env_shift) * sizeof(T);
    const int waves_per_block = waves_that_fit(per_wave);
    const unsigned used = ev.derived_used[velocity_representation];
    const jxs_obs::Shape sh{P.n_rows, P.n, velocity_representation};
    const unsigned char* b = static_cast<const unsigned char*>(ev.table);
    const EvalTable<T> tb{reinterpret_cast<const int32_t*>(b), reinterpret_cast<const int32_t*>(b + ev.targets_at), reinterpret_cast<const T*>(b + ev.offset_at),
                          reinterpret_cast<const T*>(b + ev.scale_at), reinterpret_cast<const int32_t*>(b + ev.terms_at),
                          reinterpret_cast<const T*>(b + ev.term_params_at), reinterpret_cast<const int32_t*>(b + ev.conds_at),
                          reinterpret_cast<const T*>(b + ev.cond_limits_at), ev.K, ev.C, static_cast<T>(ev.reward_lo), static_cast<T>(ev.reward_hi),
                          static_cast<T>(ev.termination_reward)};
    const dim3 grid = env_grid(env_waves(N, env_shift), waves_per_block);
    with_io_type<T>(own_reward, [&](auto r) {
      using R = decltype(r);
      with_io_type<T>(own_terms, [&](auto w) {
        using TT = decltype(w);
        hipLaunchKernelGGL((jxs_env_evaluate_kernel<T, R, TT>), grid, dim3(64 * waves_per_block), waves_per_block * per_wave, s,
                           static_cast<const T*>(state), src, tb, used, sh, N, t.tile_shift, env_shift, static_cast<R*>(reward), done, fired,
                           static_cast<TT*>(terms), (long long)terms_ld, steps, max_steps);
      });
    });
    return launched(who);
  });
}

int jxs_action_create(jxs_model* model, int A, const int32_t* joints, const double* params, jxs_action** out) {
  if (const int rc = create_preamble(model, out)) return rc;
  const char* const who = "jxs_action_create";
  if (joints == nullptr || params == nullptr) return refuse(who, "null joints or params");
  return with_typed(model, [&](auto* mt) -> int {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    const int n = P.n;
    if (n < 1) return refuse(who, "the model has no joints");
    int bad = -1;
    const int err = jxs_act::table_error(joints, params, n, A, T(0), &bad);
    if (err == jxs_act::kBadWidth)
      return refuse(who, "A = " + std::to_string(A) + " outside [0, " + std::to_string(JXS_ACT_MAX_WIDTH) + "]");
    if (err != jxs_act::kOk) {
      const char* what = err == jxs_act::kBadMode     ? "unknown mode"
                         : err == jxs_act::kBadColumn ? "column outside [-1, A)"
                         : err == jxs_act::kNotFinite ? "scale, offset, kp or kd not finite in the model's dtype"
                         : err == jxs_act::kBadLimit  ? "action_clip or torque_limit negative, NaN or not finite in the model's dtype"
                                                      : "target_lo above target_hi, NaN or not finite in the model's dtype";
      return refuse(who, "joint " + std::to_string(bad) + " {" + std::to_string(joints[2 * bad]) + ", " + std::to_string(joints[2 * bad + 1]) + "}: " + what);
    }
    if (P.n_rows >= (1 << 26)) return refuse(who, "a state of 2^26 rows or more");
    auto ac = std::make_unique<jxs_action>();
    ac->dtype = model->dtype, ac->A = A, ac->n_rows = P.n_rows, ac->n_joints = n;
    ac->params_at = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16;
    std::vector<unsigned char> host(ac->params_at + (size_t)n * sizeof(jxs_act::Params<T>), 0);
    int32_t* codes = reinterpret_cast<int32_t*>(host.data());
    jxs_act::Params<T>* pr = reinterpret_cast<jxs_act::Params<T>*>(host.data() + ac->params_at);
    for (int j = 0; j < n; ++j) {
      codes[j] = jxs_act::pack_joint(joints[2 * j], joints[2 * j + 1]);
      ac->reads_actions = ac->reads_actions || joints[2 * j + 1] >= 0;
      for (int k = 0; k < jxs_act::kParams; ++k) pr[j].v[k] = static_cast<T>(params[jxs_act::kParams * j + k]);
    }
    return upload_table(std::move(ac), host, "uploading the action table", out);
  });
}
int jxs_action_destroy(jxs_action* action) { return destroy_table(action); }

int jxs_env_act(jxs_model* model, const jxs_action* action, const void* state, const void* actions, int act_dtype, int64_t act_ld,
                const void* feed_forward, void* out_tau, int N, void* stream) {
  const char* const who = "jxs_env_act";
  if (model == nullptr || action == nullptr || state == nullptr || out_tau == nullptr) return refuse(who, "null argument");
  if (N <= 0) return refuse(who, "N must be positive");
  if (act_dtype != JXS_F32 && act_dtype != JXS_F64) return refuse(who, "unknown act_dtype");
  if (act_dtype != JXS_F32 && act_dtype != model->dtype) return refuse(who, "act_dtype must be JXS_F32 or the model's dtype");
  const jxs_action& ac = *action;
  if (act_ld < ac.A) return refuse(who, "act_ld = " + std::to_string(act_ld) + " below A = " + std::to_string(ac.A));
  if (ac.reads_actions && actions == nullptr) return refuse(who, "the table reads action columns, and actions is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& P = mt->pk.P;
    if (!table_fits(ac, model->dtype, P)) return refuse(who, "the action table was created for another state layout or dtype");
    EnvTile t;
    if (const int rc = env_tile(who, mt->pk.G, P.n_rows, t)) return rc;
    const int tile = t.tile;
    const size_t ab = act_dtype == JXS_F64 ? 8 : 4;
    const void* act = ac.reads_actions ? actions : nullptr;  // (a tensor the table does not read is not looked at)
    if ((uintptr_t)state % sizeof(T) != 0 || (uintptr_t)out_tau % sizeof(T) != 0 || (uintptr_t)feed_forward % sizeof(T) != 0 || (uintptr_t)act % ab != 0)
      return refuse(who, "state, actions, feed_forward and out_tau must be aligned to their element type");
    // The widest access that the span of the n joint rows of a tile, the tile span of the state, the places of the q and qd
    // rows in it and the three block addresses allow.  (The humanoid in fp32: 23 x 2 x 4 = 184 bytes, rows at 56 and 288: 8.)
    const int wb = (int)sizeof(T), n = P.n;
    const unsigned long long q_at = (unsigned long long)jxs_act::row_q(n) * tile * wb, qd_at = (unsigned long long)jxs_act::row_qd(n) * tile * wb;
    const int access = std::min(jxs_env::access_bytes((unsigned long long)(uintptr_t)out_tau | (unsigned long long)(uintptr_t)feed_forward, n, tile, wb),
                                jxs_env::access_bytes((unsigned long long)(uintptr_t)state | q_at | qd_at, P.n_rows, tile, wb));
    const int env_shift = jxs_env::env_shift_for(N, t.tile_shift, knob(g_act_envs_per_wave));
    const unsigned char* tb = static_cast<const unsigned char*>(ac.table);
    const int32_t* codes = reinterpret_cast<const int32_t*>(tb);
    const jxs_act::Params<T>* params = reinterpret_cast<const jxs_act::Params<T>*>(tb + ac.params_at);
    with_io_type<T>(act_dtype == model->dtype, [&](auto a) {
      using AT = decltype(a);
      with_access<sizeof(T)>(access, [&](auto width) {
        hipLaunchKernelGGL((jxs_env_act_kernel<T, AT, decltype(width)::value>), env_grid(env_waves(N, env_shift)), dim3(kEnvBlock), 0, s,
                           static_cast<const T*>(state), static_cast<const AT*>(act), (long long)act_ld, codes, params,
                           static_cast<const T*>(feed_forward), static_cast<T*>(out_tau), ac.n_joints, ac.n_rows, N, t.tile_shift, env_shift);
      });
    });
    return launched(who);
  });
}

int jxs_contact_sensors_create(jxs_model* model, int G, const int32_t* groups, int P, const int32_t* parent_link, const double* L_p,
                               jxs_contact_sensors** out) {
  if (const int rc = create_preamble(model, out)) return rc;
  const char* const who = "jxs_contact_sensors_create";
  return with_typed(model, [&](auto* mt) -> int {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& KP = mt->pk.P;
    int bad = -1;
    const int err = jxs_contact::table_error(G, groups, P, parent_link, L_p, KP.nL, sizeof(T) == 4, &bad);
    if (err == jxs_contact::kBadSize)
      return refuse(who, "G = " + std::to_string(G) + ", P = " + std::to_string(P) + " outside [1, " + std::to_string(JXS_CONTACT_MAX_GROUPS) + "], [1, " +
                             std::to_string(JXS_CONTACT_MAX_POINTS) + "], or a null table");
    if (err != jxs_contact::kOk) {
      const std::string at = std::to_string(bad);
      switch (err) {
        case jxs_contact::kBadGroup: return refuse(who, "group " + at + ": an empty range, one outside the table or one that overlaps an earlier group's");
        case jxs_contact::kUncovered: return refuse(who, "entry " + at + " belongs to no group");
        case jxs_contact::kBadParent: return refuse(who, "entry " + at + ": parent link " + std::to_string(parent_link[bad]) + " outside [0, " + std::to_string(KP.nL) + ")");
        default: return refuse(who, "entry " + at + ": L_p not finite in the model's dtype");
      }
    }
    auto cs = std::make_unique<jxs_contact_sensors>();
    cs->dtype = model->dtype, cs->G = G, cs->P = P, cs->n_rows = KP.n_rows, cs->n_joints = KP.n, cs->n_links = KP.nL;
    cs->parent_at = ((size_t)G * 2 * sizeof(int32_t) + 15) / 16 * 16;
    cs->points_at = cs->parent_at + ((size_t)P * sizeof(int32_t) + 15) / 16 * 16;
    std::vector<unsigned char> host(cs->points_at + (size_t)P * 3 * sizeof(T), 0);
    int32_t* gr = reinterpret_cast<int32_t*>(host.data());
    int32_t* pa = reinterpret_cast<int32_t*>(host.data() + cs->parent_at);
    T* pt = reinterpret_cast<T*>(host.data() + cs->points_at);
    for (int i = 0; i < 2 * G; ++i) gr[i] = groups[i];
    for (int k = 0; k < P; ++k) pa[k] = parent_link[k];
    for (int i = 0; i < 3 * P; ++i) pt[i] = static_cast<T>(L_p[i]);
    return upload_table(std::move(cs), host, "uploading the contact-sensor table", out);
  });
}
int jxs_contact_sensors_destroy(jxs_contact_sensors* sensors) { return destroy_table(sensors); }

int jxs_env_contacts(jxs_model* model, const jxs_contact_sensors* sensors, const void* link_transforms, const void* link_velocities, int N, double dt,
                     const uint8_t* reset_mask, void* timers, void* out_record, void* stream) {
  const char* const who = "jxs_env_contacts";
  if (model == nullptr || sensors == nullptr || link_transforms == nullptr || out_record == nullptr) return refuse(who, "null argument");
  if (N <= 0) return refuse(who, "N must be positive");
  const jxs_contact_sensors& cs = *sensors;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_typed(model, [&](auto* mt) {
    using T = typename std::remove_pointer_t<decltype(mt)>::value_type;
    const auto& KP = mt->pk.P;
    if (!(dt >= 0.0) || !jxs_obs::affine_ok(dt, T(0))) return refuse(who, "dt must be finite in the model's dtype and not negative");
    if (!table_fits(cs, model->dtype, KP) || cs.n_links != KP.nL) return refuse(who, "the contact-sensor table was created for another model layout or dtype");
    EnvTile t;
    if (const int rc = env_tile(who, mt->pk.G, std::max(12 * KP.nL, jxs_contact::kRows * cs.G), t)) return rc;
    if ((uintptr_t)link_transforms % sizeof(T) != 0 || (uintptr_t)link_velocities % sizeof(T) != 0 || (uintptr_t)timers % sizeof(T) != 0 ||
        (uintptr_t)out_record % sizeof(T) != 0)
      return refuse(who, "link_transforms, link_velocities, timers and out_record must be aligned to their element type");
    // Environments per wave: one tile, whatever N, asked of the shared rule as its `want` (the knob overrides it).  The lanes
    // of this kernel run over points x environments, so a wave is full with one tile of a legged robot's table and more
    // environments only add passes: measured (profiles/env_contact.txt), a wave of 8 -- what the rule gives at N = 65 536 --
    // takes 1.5 x the time of one of 2 or 4 on the humanoid's 40 points, 16 and 32 take 2.8 x
    const int want = knob(g_contact_envs_per_wave);
    const int env_shift = jxs_env::env_shift_for(N, t.tile_shift, want > 0 ? want : t.tile);
    // points per chunk: 512 items (chunk * E) at the most; 2 * chunk * E + 3 * G * E words per wave (the worst case, 32 groups
    // of 64 fp64 environments, is 56 KB for one wave)
    const int chunk = std::max(1, std::min(cs.P, 512 >> env_shift));
    const size_t per_wave = (size_t)((2 * chunk + 3 * cs.G) << env_shift) * sizeof(T);
    const int waves_per_block = waves_that_fit(per_wave);
    const unsigned char* b = static_cast<const unsigned char*>(cs.table);
    const ContactTable<T> tb{reinterpret_cast<const int32_t*>(b), reinterpret_cast<const int32_t*>(b + cs.parent_at), reinterpret_cast<const T*>(b + cs.points_at),
                             cs.G, cs.P};
    // the terrain is the model's own: its parameters from the host copy of the model block, its samples from the device one
    jxs_contact::Terrain<T> tr{};
    tr.kind = KP.hf ? jxs_contact::kTerrainField : KP.flat ? jxs_contact::kTerrainFlat : jxs_contact::kTerrainPlane;
    tr.height = KP.terrain_h;
    for (int k = 0; k < 3; ++k) tr.normal[k] = KP.nrm[k];
    tr.inv_nz = T(1) / KP.nrm[2];
    tr.nx = KP.hf_nx, tr.ny = KP.hf_ny, tr.x0 = KP.hf_x0, tr.y0 = KP.hf_y0, tr.idx = KP.hf_idx, tr.idy = KP.hf_idy;
    tr.delta = KP.hf_delta, tr.inv_2delta = KP.hf_inv_2delta;
    tr.samples = reinterpret_cast<const T*>(mt->mblk + KP.hf_off);
    const dim3 grid = env_grid(env_waves(N, env_shift), waves_per_block);
    hipLaunchKernelGGL((jxs_env_contacts_kernel<T>), grid, dim3(64 * waves_per_block), waves_per_block * per_wave, s, static_cast<const T*>(link_transforms),
                       static_cast<const T*>(link_velocities), tb, tr, KP.nL, N, t.tile_shift, env_shift, chunk, static_cast<T>(dt), reset_mask,
                       static_cast<T*>(timers), static_cast<T*>(out_record));
    return launched(who);
  });
}

}  // extern "C"
