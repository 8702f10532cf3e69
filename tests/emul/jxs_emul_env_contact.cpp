// TEST INFRASTRUCTURE: host harness of the contact sensors (jxs_env_contacts of jaxsim_amd/csrc/jxs_env.hip).
// It drives jxs_contact::sense_env of jaxsim_amd/csrc/jxs_env_contact.h -- the function the device kernel's pieces make up --
// over EVERY environment on the CPU, reading and writing the tiled blocks through the index functions of jxs_env_ops.h, and
// writes the padding columns of the record as zero, so that tests/test_env_contact_cpu.py can compare it with the NumPy
// restatement (tests/env_contact_ref.py).  Built by tests/env_emul_lib.py with g++.
#include <cstdint>
#include <vector>

#include "jxs_env_contact.h"

namespace {

struct Terrain {
  int kind;
  double height, normal[3];
  int nx, ny;
  double origin[2], spacing[2], delta;
  const double* samples;
};

template <typename T>
void sense_all(const Terrain& t, int G, const int32_t* groups, int P, const int32_t* parent, const double* L_p, int n_links, const T* link_H, const T* link_V,
               int N, int tile, double dt, const uint8_t* reset_mask, T* timers, T* out) {
  std::vector<T> samples((size_t)(t.kind == jxs_contact::kTerrainField ? t.nx * t.ny : 0)), points(3 * (size_t)P);
  for (size_t i = 0; i < samples.size(); ++i) samples[i] = (T)t.samples[i];
  for (size_t i = 0; i < points.size(); ++i) points[i] = (T)L_p[i];
  // the parameters as jxs_pack.h rounds them into the model block
  jxs_contact::Terrain<T> tr{};
  tr.kind = t.kind, tr.height = (T)t.height;
  for (int k = 0; k < 3; ++k) tr.normal[k] = (T)t.normal[k];
  tr.inv_nz = T(1) / tr.normal[2];
  tr.nx = t.nx, tr.ny = t.ny, tr.x0 = (T)t.origin[0], tr.y0 = (T)t.origin[1];
  tr.idx = (T)(1.0 / t.spacing[0]), tr.idy = (T)(1.0 / t.spacing[1]);
  tr.delta = (T)t.delta, tr.inv_2delta = (T)(1.0 / (2.0 * t.delta));
  tr.samples = samples.data();
  const jxs_contact::Table<T> tb{G, P, groups, parent, points.data()};
  const int rows_H = 12 * n_links, rows_V = 6 * n_links, rows_out = jxs_contact::kRows * G, rows_t = jxs_contact::kTimerRows * G;
  const long long columns = jxs_env::n_tiles(N, tile) * tile;
  for (long long env = 0; env < columns; ++env) {
    if (jxs_env::is_padding(env, N)) {
      for (int r = 0; r < rows_out; ++r) out[jxs_env::word_of(env, r, rows_out, tile)] = T(0);
      continue;
    }
    jxs_contact::sense_env<T>(
        tr, tb, link_V != nullptr, timers != nullptr, reset_mask != nullptr && reset_mask[env] != 0, (T)dt,
        [&](int l, int r) { return link_H[jxs_env::word_of(env, 12 * l + r, rows_H, tile)]; },
        [&](int l, int r) { return link_V[jxs_env::word_of(env, 6 * l + r, rows_V, tile)]; },
        [&](int r) { return timers + jxs_env::word_of(env, r, rows_t, tile); }, [&](int r, T x) { out[jxs_env::word_of(env, r, rows_out, tile)] = x; });
  }
}

}  // namespace

extern "C" {

struct jxs_emul_contact_terrain {
  int32_t kind;  // 0 flat, 1 plane, 2 height field
  double height, normal[3];
  int32_t nx, ny;
  double origin[2], spacing[2], delta;
  const double* samples;
};

// kOk (0) or the error of jxs_contact::table_error, with the group or entry it is in
int jxs_emul_contact_table_error(int G, const int32_t* groups, int P, const int32_t* parent, const double* L_p, int n_links, int word_bytes, int* bad) {
  return jxs_contact::table_error(G, groups, P, parent, L_p, n_links, word_bytes == 4, bad);
}

// -1: bad word size, -2: an invalid table, a null block, N <= 0 or a dt that is negative or not finite
int jxs_emul_env_contacts(const jxs_emul_contact_terrain* t, int G, const int32_t* groups, int P, const int32_t* parent, const double* L_p, int n_links,
                          const void* link_H, const void* link_V, int N, int tile, double dt, const uint8_t* reset_mask, void* timers, void* out,
                          int word_bytes) {
  int bad;
  if (jxs_contact::table_error(G, groups, P, parent, L_p, n_links, word_bytes == 4, &bad) != jxs_contact::kOk) return -2;
  if (link_H == nullptr || out == nullptr || N <= 0 || !(dt >= 0.0) || !(word_bytes == 4 ? jxs_obs::affine_ok(dt, 0.0f) : jxs_obs::affine_ok(dt, 0.0))) return -2;
  const Terrain tr{t->kind, t->height, {t->normal[0], t->normal[1], t->normal[2]}, t->nx, t->ny, {t->origin[0], t->origin[1]}, {t->spacing[0], t->spacing[1]},
                   t->delta, t->samples};
  if (word_bytes == 4)
    sense_all<float>(tr, G, groups, P, parent, L_p, n_links, static_cast<const float*>(link_H), static_cast<const float*>(link_V), N, tile, dt, reset_mask,
                     static_cast<float*>(timers), static_cast<float*>(out));
  else if (word_bytes == 8)
    sense_all<double>(tr, G, groups, P, parent, L_p, n_links, static_cast<const double*>(link_H), static_cast<const double*>(link_V), N, tile, dt, reset_mask,
                      static_cast<double*>(timers), static_cast<double*>(out));
  else
    return -1;
  return 0;
}

}  // extern "C"
