// Host-side plumbing that the two C-ABI translation units share (jxs_api.hip: models, step, queries, device wrappers;
// jxs_env.hip: the per-environment operations).  Host only: no kernel, and nothing jxs_inst.hip or jxs_spec.hip includes.
// What has state -- the error string of the thread, the developer knobs -- is DEFINED once, in jxs_api.hip, and declared
// here: jxs_last_error and jxs_debug_reload_env reach what either unit set.  The names stay inside the library (hidden).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "jxs_pack.h"

namespace jxs_host __attribute__((visibility("hidden"))) {

// the error of an entry point: its text for jxs_last_error of this thread, its code for the caller
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#define JXS_HIP(call)                                  \
  do {                                                 \
    hipError_t e_ = (call);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #call);  \
  } while (0)

// Developer knobs (jxs_api.hip load_knobs): one of them, after the read of the environment on the first call of the process
extern std::atomic<int> g_observe_envs_per_wave, g_act_envs_per_wave, g_evaluate_envs_per_wave, g_contact_envs_per_wave;
int knob(const std::atomic<int>& k);
void debug_knobs(int& knobs, int& duo_max_blocks);

// Host tables of one model + its device model block (jxs_params.h: KParams | ltf | lti | rti | point chunks)
template <typename T>
struct ModelT {
  using value_type = T;
  jxs::Packed<T> pk;
  unsigned char* mblk = nullptr;
  // model-specialised kernels (jxs_model_attach_specialized): launch entry per mode, null = generic kernel
  using SpecLaunch = int (*)(const void*, const unsigned char*, const void*, void*);
  SpecLaunch spec_launch[jxs::kNumModes] = {};
  void* spec_handle[jxs::kNumModes] = {};
  int* faults = nullptr;  // [2] discarded contact-force / impact solves since the last reset (rigid contact models)
  // jxs_rollout_controlled, one launch per step: the torques of the current step, [n][N] -- one block per stream
  std::mutex scratch_mu;
  std::map<hipStream_t, std::pair<void*, size_t>> tau_scratch;

  ~ModelT() {
    // The specialised-kernel objects are NOT unloaded (attach_typed): launches of this model may still be in
    // flight on some stream, and unloading a code object under a running kernel is undefined; hipFree
    // synchronises the device.  The objects stay mapped for the life of the process (a few hundred KB each),
    // which also keeps them visible in /proc/self/maps to whoever audits which native code ran.
    (void)hipFree(mblk);
    (void)hipFree(faults);
    for (auto& kv : tau_scratch)
      if (kv.second.first != nullptr) (void)hipFree(kv.second.first);
  }

  hipError_t upload_all() {
    const std::vector<unsigned char> b = pk.block();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&mblk), b.size());
    if (e != hipSuccess) return e;
    if ((e = hipMemcpy(mblk, b.data(), b.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&faults), 2 * sizeof(int))) != hipSuccess) return e;
    return hipMemset(faults, 0, 2 * sizeof(int));
  }
  jxs::KArgs<T> args(int N) const {
    jxs::KArgs<T> a{};
    a.N = N;
    a.faults = faults;
    debug_knobs(a.knobs, a.duo_max_blocks);
    return a;
  }
};

}  // namespace jxs_host

struct jxs_model {
  unsigned long long uid = 0;  // unique per created model: cached launch graphs are keyed by it, not by the address
  int dtype = JXS_F32;
  std::unique_ptr<jxs_host::ModelT<float>> f32;
  std::unique_ptr<jxs_host::ModelT<double>> f64;
};

namespace jxs_host __attribute__((visibility("hidden"))) {

// the one fork on the precision: f(double{}) or f(float{}) for a dtype of the header, f(ModelT<double>*) or
// f(ModelT<float>*) for a model -- both calls of the same return type
template <typename F>
auto with_dtype(int dtype, F&& f) {
  return dtype == JXS_F64 ? f(double{}) : f(float{});
}
template <typename Model, typename F>
auto with_typed(Model* model, F&& f) {
  return model->dtype == JXS_F64 ? f(model->f64.get()) : f(model->f32.get());
}

// a tile-interleaved [rows][N] block: N rounded up to whole tiles of 64 / G environments
inline size_t n_tiles(int N, int tile) { return (size_t)((N + tile - 1) / tile); }
inline size_t tiled_elems(int N, int tile, size_t rows) { return n_tiles(N, tile) * tile * rows; }
template <typename T>
size_t tiled_bytes(const ModelT<T>* mt, int N, size_t rows) { return sizeof(T) * tiled_elems(N, 64 / mt->pk.G, rows); }
inline size_t tiled_bytes(const jxs_model* model, int N, size_t rows) {
  return with_typed(model, [&](auto* mt) { return tiled_bytes(mt, N, rows); });
}

}  // namespace jxs_host
