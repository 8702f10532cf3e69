// TEST INFRASTRUCTURE: CPU lockstep emulation of MODE_FD_CRB (jaxsim_amd/csrc/jxs_core.h Core::fd_crb).
//
// A translation unit of its own next to jxs_emul.cpp, like jxs_emul_coriolis.cpp: it instantiates the kernel core for
// this one mode only (float and double, every lane-group size).  The host lanes get exactly the LDS words per
// environment the device launch allocates (jxs_params.h fdcrb_lds_words_per_env) as their limit: an access beyond it is
// reported as an error, so the row arithmetic of the factorisation is checked on the CPU.  The caller prepares the
// output (the tests fill it with NaN: the kernel writes every entry).  Built by tests/fd_crb_emul.py.
#include <string>

#include "jxs_lanes_host.h"
// lanes first: the core's unqualified calls on Vec resolve by ADL
#include "../../jaxsim_amd/csrc/jxs_core.h"
#include "../../jaxsim_amd/csrc/jxs_pack.h"

namespace {

thread_local std::string g_err;

template <typename T, int G>
void run_group(const jxs::Packed<T>& pk, jxs::KArgs<T> a) {
  a.ltf = pk.ltf.data();
  a.lti = pk.lti_packed.data();
  a.chunks = pk.chunks.data();
  a.rti = pk.rti_packed.data();
  a.hf = pk.hf.empty() ? nullptr : pk.hf.data();
  a.has_lds = 0;
  const size_t words = (size_t)jxs::fdcrb_lds_words_per_env(pk.P.nL, pk.P.max_depth);
  for (int env = 0; env < a.N; ++env) {
    jxs::HostLanes<T, G> ln(a.N, env, words, words);
    jxs::Core<jxs::HostLanes<T, G>> core(pk.P, a, ln);
    core.template run<jxs::MODE_FD_CRB>();
    if (ln.lds_oob_ >= 0) g_err = "MODE_FD_CRB touched LDS word " + std::to_string(ln.lds_oob_) + " of " + std::to_string(words) + " allocated";
  }
}

template <typename T>
int run_typed(const jxs_model_desc* d, const void* state, const void* tau, const void* link_f, int force_repr, void* out_acc, int N) {
  jxs::Packed<T> pk;
  const std::string err = jxs::pack_model<T>(*d, pk);
  if (!err.empty()) {
    g_err = err;
    return JXS_EINVAL;
  }
  jxs::KArgs<T> a{};
  a.state_in = static_cast<const T*>(state);
  a.tau = static_cast<const T*>(tau);
  a.link_f = static_cast<const T*>(link_f);
  a.force_repr = force_repr;
  a.out_a = static_cast<T*>(out_acc);
  a.N = N;
  a.n_steps = 1;
  g_err.clear();
  switch (pk.G) {
    case 4: run_group<T, 4>(pk, a); break;
    case 8: run_group<T, 8>(pk, a); break;
    case 16: run_group<T, 16>(pk, a); break;
    case 32: run_group<T, 32>(pk, a); break;
    case 64: run_group<T, 64>(pk, a); break;
    default: g_err = "bad group size"; return JXS_EINVAL;
  }
  return g_err.empty() ? JXS_OK : JXS_EINVAL;
}

}  // namespace

extern "C" {

const char* jxs_emul_fd_crb_last_error(void) { return g_err.c_str(); }

int jxs_emul_fd_crb(const jxs_model_desc* d, const void* state, const void* tau, const void* link_f, int force_repr, void* out_acc, int N) {
  return d->dtype == JXS_F64 ? run_typed<double>(d, state, tau, link_f, force_repr, out_acc, N)
                             : run_typed<float>(d, state, tau, link_f, force_repr, out_acc, N);
}
}
