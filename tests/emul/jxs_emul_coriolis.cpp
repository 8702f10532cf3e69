// TEST INFRASTRUCTURE: CPU lockstep emulation of MODE_CORIOLIS (jaxsim_amd/csrc/jxs_core.h Core::coriolis).
//
// A translation unit of its own next to jxs_emul.cpp, like jxs_emul_frames.cpp: it instantiates the kernel core for this
// one mode only (float and double, every lane-group size).  Like the device launch the mode gets no LDS: the host lanes
// are given an allocation limit of zero words, and any LDS access of the mode is reported as an error.  The caller
// prepares the outputs (jxs_coriolis zeroes them; the tests fill them with NaN to see which entries the kernel writes).
// Built by tests/coriolis_emul.py.
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
  for (int env = 0; env < a.N; ++env) {
    jxs::HostLanes<T, G> ln(a.N, env, 0, 0);
    jxs::Core<jxs::HostLanes<T, G>> core(pk.P, a, ln);
    core.template run<jxs::MODE_CORIOLIS>();
    if (ln.lds_oob_ >= 0) g_err = "MODE_CORIOLIS touched the LDS (word " + std::to_string(ln.lds_oob_) + "): the launch allocates none";
  }
}

template <typename T>
int run_typed(const jxs_model_desc* d, const void* state, void* out_C, void* out_M, int N) {
  jxs::Packed<T> pk;
  const std::string err = jxs::pack_model<T>(*d, pk);
  if (!err.empty()) {
    g_err = err;
    return JXS_EINVAL;
  }
  jxs::KArgs<T> a{};
  a.state_in = static_cast<const T*>(state);
  a.out_a = static_cast<T*>(out_C);
  a.out_H = static_cast<T*>(out_M);
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

const char* jxs_emul_coriolis_last_error(void) { return g_err.c_str(); }

int jxs_emul_coriolis(const jxs_model_desc* d, const void* state, void* out_C, void* out_M, int N) {
  return d->dtype == JXS_F64 ? run_typed<double>(d, state, out_C, out_M, N) : run_typed<float>(d, state, out_C, out_M, N);
}
}
