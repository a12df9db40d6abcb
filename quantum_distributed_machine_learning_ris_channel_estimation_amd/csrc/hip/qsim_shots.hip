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
#include "common.h"

namespace qd {
namespace qshots {

struct cf {
  float x, y;
};
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int kMaxQubits = 12;
constexpr int kMaxShots = 1 << 20;

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

template <int N>
__device__ __forceinline__ int ring_inv(int k) {
  k ^= (k >> (N - 1)) & 1;
#pragma unroll
  for (int i = N - 2; i >= 0; --i) k ^= ((k >> i) & 1) << (i + 1);
  return k;
}

// (cos, sin) of theta/2 and (cos, sin) of phi/2 of one layer's qubits, into LDS
__device__ __forceinline__ void layer_trig(float4* trig, const float* wl, const float* xs, int n) {
  if (threadIdx.x < n) {
    const int q = threadIdx.x;
    float s, c, sp, cp;
    __sincosf(0.5f * (wl[2 * q] + (xs ? xs[q] : 0.f)), &s, &c);
    __sincosf(0.5f * wl[2 * q + 1], &sp, &cp);
    trig[q] = make_float4(c, s, cp, sp);
  }
}

// RZ(phi) RY(theta) on the pair (a0: bit 0, a1: bit 1)
__device__ __forceinline__ void gate_fwd(cf& a0, cf& a1, float4 t) {
  const cf t0 = {t.x * a0.x - t.y * a1.x, t.x * a0.y - t.y * a1.y};
  const cf t1 = {t.y * a0.x + t.x * a1.x, t.y * a0.y + t.x * a1.y};
  a0 = cmul(t0, cf{t.z, -t.w});
  a1 = cmul(t1, cf{t.z, t.w});
}

// The circuit's final state of one sample, in A (LDS).
template <int N>
__device__ void build_state(cf* A, float4* trig, const float* xs, const float* w, int L) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;   // amplitudes per thread of the ring pass
  layer_trig(trig, w, xs, N);
  __syncthreads();
  // embedding + layer 0 + ring: the product state gathered through f^-1
  for (int j = threadIdx.x; j < D; j += NT) {
    const int k = ring_inv<N>(j);
    cf a = {1.f, 0.f};
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const float4 t = trig[q];
      a = cmul(a, ((k >> q) & 1) ? cf{t.y * t.z, t.y * t.w} : cf{t.x * t.z, -t.x * t.w});
    }
    A[j] = a;
  }
  __syncthreads();
  for (int l = 1; l < L; ++l) {
    layer_trig(trig, w + 2 * N * l, nullptr, N);
    __syncthreads();
    // pair sweeps, up to three qubits per LDS round trip: a thread owns the 2^NB amplitudes that differ in the
    // group's bits (the layer's gates act on different wires, so they commute)
    static_for<0, (N + 2) / 3>([&](auto gc) {
      constexpr int g0 = 3 * decltype(gc)::value;
      constexpr int NB = (N - g0) < 3 ? (N - g0) : 3;
      for (int t = threadIdx.x; t < (D >> NB); t += NT) {
        const int base = ((t >> g0) << (g0 + NB)) | (t & ((1 << g0) - 1));
        cf a[1 << NB];
#pragma unroll
        for (int j = 0; j < (1 << NB); ++j) a[j] = A[base | (j << g0)];
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
      if (j < D) a[i] = A[ring_inv<N>(j)];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = threadIdx.x + i * NT;
      if (j < D) A[j] = a[i];
    }
    __syncthreads();
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

// Draw `shots` outcomes of sample b from the scanned CDF and write E (and counts).  Every thread calls it.
template <int N>
__device__ void sample_counts(const uint32_t* cdf, uint32_t T, uint32_t* wcnt, float* __restrict__ E,
                              int* __restrict__ counts, int b, int shots, unsigned long long seed,
                              unsigned long long ctr) {
  constexpr int D = 1 << N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t acc[N];   // wave-uniform
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0;
  const uint32_t nblk = ((uint32_t)shots + 3u) >> 2;   // Philox blocks: four shots each
  for (uint32_t j0 = 0; j0 < nblk; j0 += NT) {
    const uint32_t j = j0 + threadIdx.x;
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
  if (threadIdx.x < N) {
    int c1 = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) c1 += (int)wcnt[k * N + threadIdx.x];
    E[(size_t)b * N + threadIdx.x] = __fdiv_rn((float)(shots - 2 * c1), (float)shots);
    if (counts != nullptr) counts[(size_t)b * N + threadIdx.x] = c1;
  }
}

__device__ __forceinline__ unsigned long long shot_counter(unsigned long long ctr0, const unsigned long long* counter) {
  return ctr0 + (counter != nullptr ? *counter : 0ull);
}

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

#define QD_SHOTS_DISPATCH(n, CALL)             \
  switch (n) {                                 \
    case 2: return CALL(2);                    \
    case 3: return CALL(3);                    \
    case 4: return CALL(4);                    \
    case 5: return CALL(5);                    \
    case 6: return CALL(6);                    \
    case 7: return CALL(7);                    \
    case 8: return CALL(8);                    \
    case 9: return CALL(9);                    \
    case 10: return CALL(10);                  \
    case 11: return CALL(11);                  \
    case 12: return CALL(12);                  \
    default: return (int)hipErrorInvalidValue; \
  }

static bool shots_ok(int n, int shots) { return n >= 2 && n <= kMaxQubits && shots >= 1 && shots <= kMaxShots; }

// probs (B, 2^n) fp32 = |amp_k|^2 of the circuit's final state, natural basis order.
QD_API int qd_qsim_probs(const float* x, const float* w, float* probs, int B, int n, int L, int wgroup, void* stream) {
  if (n < 2 || n > kMaxQubits || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
#define CALL_P(NN) launch_probs<NN>(x, w, probs, B, L, wgroup, (hipStream_t)stream)
  QD_SHOTS_DISPATCH(n, CALL_P)
#undef CALL_P
}

// E (B, n) fp32 and counts (B, n) int32 (nullable) from `shots` draws of every row of probs (B, 2^n) fp32, a
// normalised distribution.  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_sample_z(const float* probs, float* E, int* counts, int B, int n, int shots, unsigned long long seed,
                       unsigned long long ctr0, const void* counter, void* stream) {
  if (!shots_ok(n, shots) || B < 1) return (int)hipErrorInvalidValue;
#define CALL_S(NN) \
  launch_sample<NN>(probs, E, counts, B, shots, seed, ctr0, (const unsigned long long*)counter, (hipStream_t)stream)
  QD_SHOTS_DISPATCH(n, CALL_S)
#undef CALL_S
}

// The fused path: state -> probabilities -> shots in one launch.
QD_API int qd_qsim_shots_fwd(const float* x, const float* w, float* E, int* counts, int B, int n, int L, int wgroup,
                             int shots, unsigned long long seed, unsigned long long ctr0, const void* counter,
                             void* stream) {
  if (!shots_ok(n, shots) || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
#define CALL_F(NN)                                                                                  \
  launch_shots<NN>(x, w, E, counts, B, L, wgroup, shots, seed, ctr0, (const unsigned long long*)counter, \
                   (hipStream_t)stream)
  QD_SHOTS_DISPATCH(n, CALL_F)
#undef CALL_F
}

// *counter += delta (one thread): launched after a sampling launch, so that every replay of a captured graph draws
// fresh shots.  The sampling kernels only read the counter.
QD_API int qd_counter_add(void* counter, unsigned long long delta, void* stream) {
  if (counter == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)counter, delta);
  return (int)hipGetLastError();
}
