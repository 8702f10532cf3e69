// TEST INFRASTRUCTURE: CPU lockstep emulation of the single-launch query modes (jaxsim_amd/csrc/jxs_core.h):
// MODE_CENTROIDAL (Core::centroidal), MODE_FRAMES (Core::frames), MODE_CORIOLIS (Core::coriolis), MODE_FD_CRB (Core::fd_crb).
//
// A translation unit of its own next to jxs_emul.cpp: it instantiates the kernel core for these modes only (float and
// double, every lane-group size), so the main harness stays as it is.  Built by tests/query_emul.py.  The host lanes get
// exactly the LDS words per environment the device launch allocates (jxs_kernels.h launch_one) as their limit, and an
// access beyond it is reported as an error: zero words for the modes that get no LDS (any access is an error),
// jxs_params.h fdcrb_lds_words_per_env for MODE_FD_CRB, whose row arithmetic of the factorisation is so checked on the
// CPU.  The caller prepares the outputs (the tests fill them with NaN to see which entries a kernel writes; jxs_coriolis
// zeroes its own).
#include <string>
#include <vector>

#include "jxs_lanes_host.h"
// lanes first: the core's unqualified calls on Vec resolve by ADL
#include "../../jaxsim_amd/csrc/jxs_core.h"
#include "../../jaxsim_amd/csrc/jxs_pack.h"

namespace {

thread_local std::string g_err;

template <typename T, int G, int MODE>
void run_group(const jxs::Packed<T>& pk, jxs::KArgs<T> a, size_t lds_words) {
  a.ltf = pk.ltf.data();
  a.lti = pk.lti_packed.data();
  a.chunks = pk.chunks.data();
  a.rti = pk.rti_packed.data();
  a.hf = pk.hf.empty() ? nullptr : pk.hf.data();
  a.has_lds = 0;  // (what jxs_kernel sets for these modes)
  for (int env = 0; env < a.N; ++env) {
    jxs::HostLanes<T, G> ln(a.N, env, lds_words, lds_words);
    jxs::Core<jxs::HostLanes<T, G>> core(pk.P, a, ln);
    core.template run<MODE>();
    if (ln.lds_oob_ >= 0)
      g_err = "mode " + std::to_string(MODE) + " touched LDS word " + std::to_string(ln.lds_oob_) + " of " + std::to_string(lds_words) +
              " allocated by its launch";
  }
}

// one emulated launch of MODE on a packed model; `a` holds what the entry point set, N included
template <int MODE, typename T>
int run_mode(const jxs::Packed<T>& pk, jxs::KArgs<T> a, size_t lds_words) {
  a.n_steps = 1;
  g_err.clear();
  switch (pk.G) {
    case 4: run_group<T, 4, MODE>(pk, a, lds_words); break;
    case 8: run_group<T, 8, MODE>(pk, a, lds_words); break;
    case 16: run_group<T, 16, MODE>(pk, a, lds_words); break;
    case 32: run_group<T, 32, MODE>(pk, a, lds_words); break;
    case 64: run_group<T, 64, MODE>(pk, a, lds_words); break;
    default: g_err = "bad group size"; return JXS_EINVAL;
  }
  return g_err.empty() ? JXS_OK : JXS_EINVAL;
}

// f(packed model, zeroed KArgs with N set, T{}) in the precision T of the description
template <typename F>
int with_packed(const jxs_model_desc* d, int N, F&& f) {
  auto typed = [&](auto zero) -> int {
    using T = decltype(zero);
    jxs::Packed<T> pk;
    const std::string err = jxs::pack_model<T>(*d, pk);
    if (!err.empty()) {
      g_err = err;
      return JXS_EINVAL;
    }
    jxs::KArgs<T> a{};
    a.N = N;
    return f(pk, a, zero);
  };
  return d->dtype == JXS_F64 ? typed(double{}) : typed(float{});
}

}  // namespace

extern "C" {

const char* jxs_emul_query_last_error(void) { return g_err.c_str(); }

int jxs_emul_centroidal(const jxs_model_desc* d, const void* state, void* out_record, void* out_cmm, int N) {
  return with_packed(d, N, [&](const auto& pk, auto a, auto zero) {
    using T = decltype(zero);
    a.state_in = static_cast<const T*>(state);
    a.out_H = static_cast<T*>(out_record);
    a.out_a = static_cast<T*>(out_cmm);
    return run_mode<jxs::MODE_CENTROIDAL>(pk, a, 0);
  });
}

// the target table is built the way jxs_frames_create builds it (parent lane from the packer's lane table)
int jxs_emul_frames(const jxs_model_desc* d, int n, const int* parent_link, const double* L_H_F, const void* state, int in_repr,
                    int out_repr, void* out_record, void* out_J, int N) {
  return with_packed(d, N, [&](const auto& pk, auto a, auto zero) {
    using T = decltype(zero);
    std::vector<int> lane_of(pk.P.nL, -1);
    for (int l = 0; l < pk.G; ++l) {
      const int link = pk.lti[l * jxs::kLtiStride + jxs::LI_LINK];
      if (link >= 0 && link < pk.P.nL) lane_of[link] = l;
    }
    std::vector<T> tgt((size_t)n * jxs::kTgtStride, T(0));
    for (int t = 0; t < n; ++t) {
      T* r = tgt.data() + (size_t)t * jxs::kTgtStride;
      r[jxs::TG_LANE] = static_cast<T>(lane_of[parent_link[t]]);
      r[jxs::TG_LINK] = static_cast<T>(parent_link[t]);
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r[jxs::TG_R + 3 * i + j] = static_cast<T>(L_H_F[16 * t + 4 * i + j]);
        r[jxs::TG_P + i] = static_cast<T>(L_H_F[16 * t + 4 * i + 3]);
      }
    }
    a.state_in = static_cast<const T*>(state);
    a.out_H = static_cast<T*>(out_record);
    a.out_a = static_cast<T*>(out_J);
    a.tgt = tgt.data();
    a.n_tgt = n;
    a.in_repr = in_repr;
    a.out_repr = out_repr;
    return run_mode<jxs::MODE_FRAMES>(pk, a, 0);
  });
}

int jxs_emul_coriolis(const jxs_model_desc* d, const void* state, void* out_C, void* out_M, int N) {
  return with_packed(d, N, [&](const auto& pk, auto a, auto zero) {
    using T = decltype(zero);
    a.state_in = static_cast<const T*>(state);
    a.out_a = static_cast<T*>(out_C);
    a.out_H = static_cast<T*>(out_M);
    return run_mode<jxs::MODE_CORIOLIS>(pk, a, 0);
  });
}

int jxs_emul_fd_crb(const jxs_model_desc* d, const void* state, const void* tau, const void* link_f, int force_repr, void* out_acc, int N) {
  return with_packed(d, N, [&](const auto& pk, auto a, auto zero) {
    using T = decltype(zero);
    a.state_in = static_cast<const T*>(state);
    a.tau = static_cast<const T*>(tau);
    a.link_f = static_cast<const T*>(link_f);
    a.force_repr = force_repr;
    a.out_a = static_cast<T*>(out_acc);
    return run_mode<jxs::MODE_FD_CRB>(pk, a, (size_t)jxs::fdcrb_lds_words_per_env(pk.P.nL, pk.P.max_depth));
  });
}
}
