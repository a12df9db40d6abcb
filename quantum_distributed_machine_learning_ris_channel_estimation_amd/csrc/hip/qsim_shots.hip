// Finite-shot measurement of the QSC circuit (n = 2 .. 12): one 256-thread workgroup per sample, the state and the
// sampling CDF LDS-resident.  The CNOT ring's gather goes through registers (its buffer is the register file) and
// the CDF is built over the state it replaces, so a workgroup holds one state (32 KiB at n = 12): four per CU.
//
// Same circuit as csrc/hip/qsim.hip / qsim_big.hip (RY embedding, L x [RY, RZ on every wire, CNOT ring]); wire i is
// bit i of the basis index.  Three kernels share the device functions below:
//   qsim_probs_kernel   state -> |amp_k|^2 (fp32, natural basis order) to HBM
//   sample_z_kernel     fp32 probabilities from HBM -> shots -> E / counts
//   qsim_shots_kernel   state -> probabilities -> shots in one launch; only E / counts go to HBM
//
// Sampling contract (csrc/cpu/qsim_cpu.cpp qd_cpu_sample_z implements the same, sequentially; everything after the
// fp32 probability is integer, so the two agree bit for bit whatever the scan order):
//   q_k  = (uint32) rint(p_k * 2^30)              (exact product, round to nearest even; non-positive / NaN -> 0)
//   cum  = inclusive prefix sum of q (uint32), T = cum[2^n - 1]   (a normalised p gives T <= 2^30 + 2^11)
//   shot s of sample b: r = word (s & 3) of Philox4x32-10(counter (s >> 2, b, lo32(c), hi32(c)), key (lo32(seed),
//                       hi32(seed))), c = ctr0 + (counter ? *counter : 0)
//   t = (uint64(r) * T) >> 32; outcome k = the smallest index with cum[k] > t (never a zero-probability outcome)
//   c1[i] = shots whose outcome has bit i set;  E[b, i] = (float)(shots - 2 c1[i]) / (float)shots
#include "qsim_shots_dev.h"

namespace qd {
namespace qshots {

// ------------------------------------------------------------------------------- kernels
template <int N>
__global__ void __launch_bounds__(NT) qsim_probs_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ probs, int L, int wgroup) {
  constexpr int D = 1 << N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  cf* A = reinterpret_cast<cf*>(smem + O_DATA);
  const int b = blockIdx.x;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * 2 * N * L : 0);
  build_state<N>(A, trig, x + (size_t)b * N, wsmp, L);
  for (int k = threadIdx.x; k < D; k += NT) probs[(size_t)b * D + k] = prob_of(A[k]);
}

template <int N>
__global__ void __launch_bounds__(NT) sample_z_kernel(const float* __restrict__ probs, float* __restrict__ E,
                                                      int* __restrict__ counts, int shots, unsigned long long seed,
                                                      unsigned long long ctr0,
                                                      const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  uint32_t* cdf = reinterpret_cast<uint32_t*>(smem + O_DATA);
  const int b = blockIdx.x;
  for (int k = threadIdx.x; k < D; k += NT) cdf[cdf_at(k)] = quantise(probs[(size_t)b * D + k]);
  const uint32_t T = cdf_scan<N>(cdf, wtot);
  sample_counts<N>(cdf, T, wcnt, E, counts, b, shots, seed, shot_counter(ctr0, counter));
}

template <int N>
__global__ void __launch_bounds__(NT) qsim_shots_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ E, int* __restrict__ counts, int L,
                                                        int wgroup, int shots, unsigned long long seed,
                                                        unsigned long long ctr0,
                                                        const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  cf* A = reinterpret_cast<cf*>(smem + O_DATA);
  uint32_t* cdf = reinterpret_cast<uint32_t*>(smem + O_DATA);   // over the state, once it has been read
  constexpr int PER = D >= NT ? D / NT : 1;
  const int b = blockIdx.x;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * 2 * N * L : 0);
  build_state<N>(A, trig, x + (size_t)b * N, wsmp, L);
  uint32_t q[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = threadIdx.x + i * NT;
    if (k < D) q[i] = quantise(prob_of(A[k]));
  }
  __syncthreads();   // every amplitude has been read: the CDF may overwrite the state
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = threadIdx.x + i * NT;
    if (k < D) cdf[cdf_at(k)] = q[i];
  }
  const uint32_t T = cdf_scan<N>(cdf, wtot);
  sample_counts<N>(cdf, T, wcnt, E, counts, b, shots, seed, shot_counter(ctr0, counter));
}

__global__ void counter_add_kernel(unsigned long long* counter, unsigned long long delta) { *counter += delta; }

template <int N>
static int launch_probs(const float* x, const float* w, float* probs, int B, int L, int wgroup, hipStream_t st) {
  const size_t sm = smem_bytes<N>(true);
  if (hipError_t e = allow_lds(qsim_probs_kernel<N>, sm)) return (int)e;
  hipLaunchKernelGGL(qsim_probs_kernel<N>, dim3(B), dim3(NT), sm, st, x, w, probs, L, wgroup);
  return (int)hipGetLastError();
}
template <int N>
static int launch_sample(const float* probs, float* E, int* counts, int B, int shots, unsigned long long seed,
                         unsigned long long ctr0, const unsigned long long* counter, hipStream_t st) {
  const size_t sm = smem_bytes<N>(false);
  hipLaunchKernelGGL(sample_z_kernel<N>, dim3(B), dim3(NT), sm, st, probs, E, counts, shots, seed, ctr0, counter);
  return (int)hipGetLastError();
}
template <int N>
static int launch_shots(const float* x, const float* w, float* E, int* counts, int B, int L, int wgroup, int shots,
                        unsigned long long seed, unsigned long long ctr0, const unsigned long long* counter,
                        hipStream_t st) {
  const size_t sm = smem_bytes<N>(true);
  if (hipError_t e = allow_lds(qsim_shots_kernel<N>, sm)) return (int)e;
  hipLaunchKernelGGL(qsim_shots_kernel<N>, dim3(B), dim3(NT), sm, st, x, w, E, counts, L, wgroup, shots, seed, ctr0,
                     counter);
  return (int)hipGetLastError();
}

}  // namespace qshots
}  // namespace qd

using namespace qd::qshots;

static bool shots_ok(int n, int shots) { return n >= 2 && n <= kMaxQubits && shots >= 1 && shots <= kMaxShots; }

// probs (B, 2^n) fp32 = |amp_k|^2 of the circuit's final state, natural basis order.
QD_API int qd_qsim_probs(const float* x, const float* w, float* probs, int B, int n, int L, int wgroup, void* stream) {
  if (n < 2 || n > kMaxQubits || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) { return launch_probs<N>(x, w, probs, B, L, wgroup, (hipStream_t)stream); });
}

// E (B, n) fp32 and counts (B, n) int32 (nullable) from `shots` draws of every row of probs (B, 2^n) fp32, a
// normalised distribution.  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_sample_z(const float* probs, float* E, int* counts, int B, int n, int shots, unsigned long long seed,
                       unsigned long long ctr0, const void* counter, void* stream) {
  if (!shots_ok(n, shots) || B < 1) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return launch_sample<N>(probs, E, counts, B, shots, seed, ctr0, (const unsigned long long*)counter,
                            (hipStream_t)stream);
  });
}

// The fused path: state -> probabilities -> shots in one launch.
QD_API int qd_qsim_shots_fwd(const float* x, const float* w, float* E, int* counts, int B, int n, int L, int wgroup,
                             int shots, unsigned long long seed, unsigned long long ctr0, const void* counter,
                             void* stream) {
  if (!shots_ok(n, shots) || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return launch_shots<N>(x, w, E, counts, B, L, wgroup, shots, seed, ctr0, (const unsigned long long*)counter,
                           (hipStream_t)stream);
  });
}

// *counter += delta (one thread): launched after a sampling launch, so that every replay of a captured graph draws
// fresh shots.  The sampling kernels only read the counter.
QD_API int qd_counter_add(void* counter, unsigned long long delta, void* stream) {
  if (counter == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)counter, delta);
  return (int)hipGetLastError();
}
