// Device functions of the parameter-shift kernels (qsim_pshift.hip, qsim_onchip.hip): the kept state that enters a
// layer (a second LDS buffer, or at n = 12 a thread's registers) and the final state of a circuit with one angle of
// that layer shifted.  Both kernels reach the noiseless shifted state through shifted_state below, the same inline
// pieces in the same order, so they form the same fp32 amplitudes.
#pragma once
#include "qsim_shots_dev.h"

namespace qd {
namespace qpshift {
using namespace qd::qshots;

template <int N>
constexpr bool reg_prefix() {
  return N >= 12;
}

constexpr float kHalfPi = 1.57079632679489661923f;

// qubits per LDS round trip of a layer's pair sweeps: three leave lanes idle below 512 amplitudes
template <int N>
constexpr int group_bits() {
  return N >= 9 ? 3 : 2;
}

// A thread's share of a layer's first pair sweep (qubits 0 .. NB-1): tasks t = threadIdx.x + it NT, 2^NB amplitudes
// (t << NB) | j each
template <int N>
struct FirstSweep {
  static constexpr int NB = N < group_bits<N>() ? N : group_bits<N>();
  static constexpr int TASKS = (1 << N) >> NB;
  static constexpr int TPT = TASKS >= NT ? TASKS / NT : 1;
  static constexpr int AMPS = TPT << NB;
};

// the thread's share of the state in A, into registers
template <int N>
__device__ __forceinline__ void keep_state(cf* R, const cf* A) {
  using F = FirstSweep<N>;
#pragma unroll
  for (int it = 0; it < F::TPT; ++it) {
    const int t = threadIdx.x + it * NT;
    if (t < F::TASKS) {
#pragma unroll
      for (int j = 0; j < (1 << F::NB); ++j) R[(it << F::NB) | j] = A[(t << F::NB) | j];
    }
  }
}

// the first pair sweep of a layer on the kept state, into A (what apply_layer's group 0 does from LDS); ends with a
// barrier
template <int N>
__device__ __forceinline__ void first_sweep(const cf* R, cf* A, const float4* trig) {
  using F = FirstSweep<N>;
#pragma unroll
  for (int it = 0; it < F::TPT; ++it) {
    const int t = threadIdx.x + it * NT;
    if (t < F::TASKS) {
      cf a[1 << F::NB];
#pragma unroll
      for (int j = 0; j < (1 << F::NB); ++j) a[j] = R[(it << F::NB) | j];
#pragma unroll
      for (int b = 0; b < F::NB; ++b) {
        const float4 tg = trig[b];
#pragma unroll
        for (int j = 0; j < (1 << F::NB); ++j)
          if (!((j >> b) & 1)) gate_fwd(a[j], a[j | (1 << b)], tg);
      }
#pragma unroll
      for (int j = 0; j < (1 << F::NB); ++j) A[(t << F::NB) | j] = a[j];
    }
  }
  __syncthreads();
}

// layer_trig with one angle of the layer shifted: qubit sq's RY (sk = 0) or RZ (sk = 1) angle by sh; sq < 0: none
__device__ __forceinline__ void layer_trig_shifted(float4* trig, const float* wl, const float* xs, int n, int sq, int sk,
                                                   float sh) {
  if (threadIdx.x < n) {
    const int q = threadIdx.x;
    const float th = wl[2 * q] + (xs ? xs[q] : 0.f) + (q == sq && sk == 0 ? sh : 0.f);
    const float ph = wl[2 * q + 1] + (q == sq && sk == 1 ? sh : 0.f);
    float s, c, sp, cp;
    __sincosf(0.5f * th, &s, &c);
    __sincosf(0.5f * ph, &sp, &cp);
    trig[q] = make_float4(c, s, cp, sp);
  }
}

// The state that enters layer l > 0 of the sample's circuit, into Pfx (LDS).
template <int N>
__device__ __forceinline__ void prefix_state(cf* Pfx, float4* trig, const float* wsmp, const float* xs, int l) {
  layer_trig(trig, wsmp, xs, N);
  __syncthreads();
  product_state<N>(Pfx, trig);
  for (int m = 1; m < l; ++m) {
    layer_trig(trig, wsmp + 2 * N * m, nullptr, N);
    __syncthreads();
    apply_layer<N, group_bits<N>()>(Pfx, Pfx, trig);
  }
}

// The final state, in A, of the circuit with layer l's angle (sq, sk) shifted by sh (sq < 0: the circuit itself),
// from the state that enters layer l: Pfx (LDS; n <= 11) or the thread's share pfx of it (n = 12).
template <int N>
__device__ __forceinline__ void shifted_state(cf* A, const cf* Pfx, const cf* pfx, float4* trig, const float* wsmp,
                                              const float* xs, int l, int L, int sq, int sk, float sh) {
  constexpr int GB = group_bits<N>();
  layer_trig_shifted(trig, wsmp + 2 * N * l, l == 0 ? xs : nullptr, N, sq, sk, sh);
  __syncthreads();
  if (l == 0) {
    product_state<N>(A, trig);
  } else if constexpr (reg_prefix<N>()) {
    first_sweep<N>(pfx, A, trig);
    apply_layer<N, GB, 1>(A, A, trig);
  } else {
    apply_layer<N, GB>(Pfx, A, trig);
  }
  for (int m = l + 1; m < L; ++m) {
    layer_trig(trig, wsmp + 2 * N * m, nullptr, N);
    __syncthreads();
    apply_layer<N, GB>(A, A, trig);
  }
}

}  // namespace qpshift
}  // namespace qd
