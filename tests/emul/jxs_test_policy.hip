// TEST INFRASTRUCTURE: a stand-in for another framework's policy network (tests/test_env_observe_gpu.py): one kernel that
// reads an observation tensor [N][ld] whose first 2n columns are joint positions and joint velocities and writes the PD
// torque tau[N][n] = (q0 - q) * kp - qdot * kd, every operation rounded on its own (built with -ffp-contract=off), so
// that NumPy computes the same bits on the host.  Built by tests/policy_kernel.py with hipcc for gfx950.
#include <hip/hip_runtime.h>

__global__ void jxs_test_pd_torque_kernel(const float* obs, long long ld, const float* q0, int n, int N, float kp, float kd, float* tau) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * n) return;
  const long long e = i / n;
  const int j = (int)(i % n);
  const float p = (q0[j] - obs[e * ld + j]) * kp;
  const float d = obs[e * ld + n + j] * kd;
  tau[i] = p - d;
}

extern "C" int jxs_test_pd_torque(const void* obs, long long ld, const void* q0, int n, int N, float kp, float kd, void* tau, void* stream) {
  if (obs == nullptr || q0 == nullptr || tau == nullptr || n <= 0 || N <= 0 || ld < 2 * n) return -1;
  const long long total = (long long)N * n;
  hipLaunchKernelGGL(jxs_test_pd_torque_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(obs), ld, static_cast<const float*>(q0), n, N, kp, kd, static_cast<float*>(tau));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
