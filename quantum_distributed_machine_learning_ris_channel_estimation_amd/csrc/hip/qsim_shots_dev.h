// Device functions of the finite-shot kernels (qsim_shots.hip, qsim_pshift.hip, qsim_noise.hip, qsim_onchip.hip): the
// LDS-resident state build of the QSC circuit (FRAMED: with a Pauli frame behind a layer's ring, for the noisy
// kernels), the CDF scan,
// Philox4x32-10 and the outcome search.  The sampling contract they implement is stated at the top of qsim_shots.hip.
#pragma once
#include "qsim_gates.h"

namespace qd {
namespace qshots {
using qd::cf;
using qd::cmul;
using qd::frame_sign;
using qd::gate_fwd;
using qd::layer_trig;
using qd::ring_inv;

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int kMaxQubits = 12;
constexpr int kMaxShots = 1 << 20;

// Host side of every launcher: the kernels are instantiated per qubit count, so a runtime n in 2 .. kMaxQubits becomes
// f(std::integral_constant<int, n>{}) (f returns the launch's status); hipErrorInvalidValue outside that range.
template <typename F>
static inline int dispatch_qubits(int n, F&& f) {
  switch (n) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return (int)hipErrorInvalidValue;
  }
}
static_assert(kMaxQubits == 12, "dispatch_qubits covers 2 .. kMaxQubits");

// LDS carve (bytes): trig (<= 12 float4) | wave totals of the scan (NW) | per-wave bit counts (NW x 12) | data: the
// state (2^n complex), or the CDF (2^n words + pads: never larger) -- in the fused kernel one after the other
constexpr int O_TRIG = 0, O_WTOT = 256, O_WCNT = 272, O_DATA = 512;

// CDF word of outcome k: one pad word per 32, so the scan's 16-word chunks (n = 12) fall on different banks
__device__ __host__ __forceinline__ constexpr int cdf_at(int k) { return k + (k >> 5); }
template <int N>
constexpr int cdf_bytes() {
  return (cdf_at((1 << N) - 1) + 1) * 4;
}
template <int N>
constexpr size_t smem_bytes(bool state) {
  static_assert(cdf_bytes<N>() <= (int)sizeof(cf) * (1 << N), "the CDF fits over the state");
  return O_DATA + (state ? sizeof(cf) * (1 << N) : cdf_bytes<N>());
}

// Embedding + layer 0 + ring from the layer's trig: the product state gathered through f^-1, into A (LDS).
// FRAMED (qsim_noise.hip): followed by the Pauli frame X^fa Z^fb, A'[j] = (-1)^popc(fb & (j ^ fa)) A[j ^ fa].
template <int N, bool FRAMED = false>
__device__ __forceinline__ void product_state(cf* A, const float4* trig, int fa = 0, int fb = 0) {
  constexpr int D = 1 << N;
  for (int j = threadIdx.x; j < D; j += NT) {
    const int js = FRAMED ? (j ^ fa) : j;
    const int k = ring_inv<N>(js);
    cf a = {1.f, 0.f};
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const float4 t = trig[q];
      a = cmul(a, ((k >> q) & 1) ? cf{t.y * t.z, t.y * t.w} : cf{t.x * t.z, -t.x * t.w});
    }
    A[j] = FRAMED ? frame_sign(a, fb, js) : a;
  }
  __syncthreads();
}

// One layer (its trig in LDS, visible) applied to the state in S, the result in A (S == A: in place; else S is
// left as it was).  Ends with a barrier.  GB: qubits per LDS round trip; FIRST: the first group of qubits to sweep
// (1: the caller has applied group 0's gates on its way into A).  FRAMED: the Pauli frame (fa, fb) after the ring,
// folded into the ring gather's index and sign.
template <int N, int GB = 3, int FIRST = 0, bool FRAMED = false>
__device__ __forceinline__ void apply_layer(const cf* S, cf* A, const float4* trig, int fa = 0, int fb = 0) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;   // amplitudes per thread of the ring pass
  // pair sweeps, up to GB qubits per LDS round trip: a thread owns the 2^NB amplitudes that differ in the
  // group's bits (the layer's gates act on different wires, so they commute)
  static_for<FIRST, (N + GB - 1) / GB>([&](auto gc) {
    constexpr int g0 = GB * decltype(gc)::value;
    constexpr int NB = (N - g0) < GB ? (N - g0) : GB;
    const cf* src = g0 == 0 ? S : A;   // the first group covers every amplitude
    for (int t = threadIdx.x; t < (D >> NB); t += NT) {
      const int base = ((t >> g0) << (g0 + NB)) | (t & ((1 << g0) - 1));
      cf a[1 << NB];
#pragma unroll
      for (int j = 0; j < (1 << NB); ++j) a[j] = src[base | (j << g0)];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float4 tg = trig[g0 + b];
#pragma unroll
        for (int j = 0; j < (1 << NB); ++j)
          if (!((j >> b) & 1)) gate_fwd(a[j], a[j | (1 << b)], tg);
      }
#pragma unroll
      for (int j = 0; j < (1 << NB); ++j) A[base | (j << g0)] = a[j];
    }
    __syncthreads();
  });
  // the CNOT ring, in place: A'[j] = A[f^-1(j)], every thread's amplitudes in registers across one barrier
  cf a[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = threadIdx.x + i * NT;
    if (FRAMED) {
      if (j < D) a[i] = frame_sign(A[ring_inv<N>(j ^ fa)], fb, j ^ fa);
    } else {
      if (j < D) a[i] = A[ring_inv<N>(j)];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = threadIdx.x + i * NT;
    if (j < D) A[j] = a[i];
  }
  __syncthreads();
}

// The circuit's final state of one sample, in A (LDS).
template <int N>
__device__ void build_state(cf* A, float4* trig, const float* xs, const float* w, int L) {
  layer_trig(trig, w, xs, N);
  __syncthreads();
  product_state<N>(A, trig);
  for (int l = 1; l < L; ++l) {
    layer_trig(trig, w + 2 * N * l, nullptr, N);
    __syncthreads();
    apply_layer<N>(A, A, trig);
  }
}

// |amp|^2 with explicit roundings: the probabilities kernel and the fused kernel form the same fp32 value
__device__ __forceinline__ float prob_of(cf a) { return __fmaf_rn(a.x, a.x, __fmul_rn(a.y, a.y)); }

__device__ __forceinline__ uint32_t quantise(float p) { return p > 0.f ? __float2uint_rn(p * 1073741824.f) : 0u; }

// Inclusive prefix sum of the D quantised words in cdf (in place); returns T.  Every thread of the block calls it;
// the words must have been written before the call (it starts with a barrier).
template <int N>
__device__ uint32_t cdf_scan(uint32_t* cdf, uint32_t* wtot) {
  constexpr int D = 1 << N;
  constexpr int CH = D >= NT ? D / NT : 1;   // words per thread (threads >= D own none)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  const bool own = threadIdx.x * CH < D;
  uint32_t run = 0;
  if (own) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      run += cdf[cdf_at(threadIdx.x * CH + j)];
      cdf[cdf_at(threadIdx.x * CH + j)] = run;
    }
  }
  uint32_t v = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  if (lane == 63) wtot[wv] = v;
  __syncthreads();
  uint32_t off = v - run;
  for (int k = 0; k < wv; ++k) off += wtot[k];
  if (own) {
#pragma unroll
    for (int j = 0; j < CH; ++j) cdf[cdf_at(threadIdx.x * CH + j)] += off;
  }
  __syncthreads();
  return cdf[cdf_at(D - 1)];
}

struct Philox {
  uint32_t c[4];
};
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// Draw `shots` outcomes of row b (the Philox counter's second word) from the scanned CDF; thread i < N returns
// c1[i], the others 0.  Every thread calls it; wcnt may be rewritten only after a further barrier.  IDLE_SKIP: a
// wave none of whose lanes holds a shot skips the draw (the same counts).
template <int N, bool IDLE_SKIP = false>
__device__ int shot_counts(const uint32_t* cdf, uint32_t T, uint32_t* wcnt, int b, int shots, unsigned long long seed,
                           unsigned long long ctr) {
  constexpr int D = 1 << N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t acc[N];   // wave-uniform
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0;
  const uint32_t nblk = ((uint32_t)shots + 3u) >> 2;   // Philox blocks: four shots each
  for (uint32_t j0 = 0; j0 < nblk; j0 += NT) {
    const uint32_t j = j0 + threadIdx.x;
    if (IDLE_SKIP && j0 + (uint32_t)wv * 64u >= nblk) break;   // wave-uniform
    const Philox ph = philox4x32_10(j, (uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = j < nblk && 4u * j + r < (uint32_t)shots;   // lanes beyond `shots` count nothing
      const uint32_t t = __umulhi(ph.c[r], T);
      int k = 0;   // upper bound: the smallest k with cum[k] > t (t < T = cum[D - 1] whenever T > 0)
#pragma unroll
      for (int step = D >> 1; step >= 1; step >>= 1)
        if (cdf[cdf_at(k + step - 1)] <= t) k += step;
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] += (uint32_t)__popcll(__ballot(valid && ((k >> i) & 1)));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) wcnt[wv * N + i] = acc[i];
  }
  __syncthreads();
  int c1 = 0;
  if (threadIdx.x < N) {
#pragma unroll
    for (int k = 0; k < NW; ++k) c1 += (int)wcnt[k * N + threadIdx.x];
  }
  return c1;
}

__device__ __forceinline__ float shots_mean(int c1, int shots) {
  return __fdiv_rn((float)(shots - 2 * c1), (float)shots);
}

// Draw `shots` outcomes of sample b from the scanned CDF and write E (and counts).  Every thread calls it.
template <int N>
__device__ void sample_counts(const uint32_t* cdf, uint32_t T, uint32_t* wcnt, float* __restrict__ E,
                              int* __restrict__ counts, int b, int shots, unsigned long long seed,
                              unsigned long long ctr) {
  const int c1 = shot_counts<N>(cdf, T, wcnt, b, shots, seed, ctr);
  if (threadIdx.x < N) {
    E[(size_t)b * N + threadIdx.x] = shots_mean(c1, shots);
    if (counts != nullptr) counts[(size_t)b * N + threadIdx.x] = c1;
  }
}

__device__ __forceinline__ unsigned long long shot_counter(unsigned long long ctr0, const unsigned long long* counter) {
  return ctr0 + (counter != nullptr ? *counter : 0ull);
}

}  // namespace qshots
}  // namespace qd
