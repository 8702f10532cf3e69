// TEST INFRASTRUCTURE: CPU lockstep emulation of MODE_FRAMES (jaxsim_amd/csrc/jxs_core.h Core::frames).
//
// A translation unit of its own next to jxs_emul.cpp, like jxs_emul_centroidal.cpp: it instantiates the kernel core for
// this one mode only (float and double, every lane-group size).  The target table is built the way jxs_frames_create
// builds it (parent lane from the packer's lane table).  Like the device launch the mode gets no LDS: the host lanes are
// given an allocation limit of zero words, and any LDS access of the mode is reported as an error.  Built by
// tests/frames_emul.py.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

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
    core.template run<jxs::MODE_FRAMES>();
    if (ln.lds_oob_ >= 0) g_err = "MODE_FRAMES touched the LDS (word " + std::to_string(ln.lds_oob_) + "): the launch allocates none";
  }
}

template <typename T>
int run_typed(const jxs_model_desc* d, int n, const int* parent_link, const double* L_H_F, const void* state, int in_repr,
              int out_repr, void* out_record, void* out_J, int N) {
  jxs::Packed<T> pk;
  const std::string err = jxs::pack_model<T>(*d, pk);
  if (!err.empty()) {
    g_err = err;
    return JXS_EINVAL;
  }
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
  jxs::KArgs<T> a{};
  a.state_in = static_cast<const T*>(state);
  a.out_H = static_cast<T*>(out_record);
  a.out_a = static_cast<T*>(out_J);
  a.tgt = tgt.data();
  a.n_tgt = n;
  a.in_repr = in_repr;
  a.out_repr = out_repr;
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

const char* jxs_emul_frames_last_error(void) { return g_err.c_str(); }

int jxs_emul_frames(const jxs_model_desc* d, int n, const int* parent_link, const double* L_H_F, const void* state, int in_repr,
                    int out_repr, void* out_record, void* out_J, int N) {
  return d->dtype == JXS_F64 ? run_typed<double>(d, n, parent_link, L_H_F, state, in_repr, out_repr, out_record, out_J, N)
                             : run_typed<float>(d, n, parent_link, L_H_F, state, in_repr, out_repr, out_record, out_J, N);
}
}
