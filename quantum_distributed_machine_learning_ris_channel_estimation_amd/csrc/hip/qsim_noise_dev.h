// Device functions of the noisy kernels (qsim_noise.hip, qsim_onchip.hip, qsim_nadj.hip): the Pauli frame of a layer of
// a trajectory, the framed draw of a Philox block's four shots with
// readout flips, and the state -> CDF step; and the host side the three entry points share (argument checks, chunks
// per sample).  The contract they implement is stated at the top of qsim_noise.hip.
#pragma once
#include "qsim_shots_dev.h"

namespace qd {
namespace qnoise {

using namespace qd::qshots;

constexpr int kMaxTraj = 1024;
constexpr int kMaxSites = 4096;
constexpr int kLdsBudget = 40 * 1024;   // a quarter of a CU's LDS: what a workgroup may take and still be one of four
__host__ __device__ constexpr size_t traj_bytes(int T) { return sizeof(uint16_t) * (((size_t)T + 7) & ~(size_t)7); }
constexpr uint16_t kRebuild = 0x8000;   // traj word: bit 15 = a frame before the last layer is not identity; low bits = the last layer's X mask

struct Rng {
  uint32_t b, c_lo, c_hi, k0, k1;
};

// (x, z) bits of a one-qubit Pauli code 0 .. 3 = I, X, Y, Z
__device__ __forceinline__ uint32_t pauli_x(uint32_t p) { return ((p + 1u) >> 1) & 1u; }
__device__ __forceinline__ uint32_t pauli_z(uint32_t p) { return (p >> 1) & 1u; }

// floor(r m / thr) for r < thr, without a 64-bit division: the number of multiples of thr that are <= r m
template <int M>
__device__ __forceinline__ uint32_t scaled_code(uint32_t r, uint32_t thr) {
  const unsigned long long v = (unsigned long long)r * M;
  uint32_t q = 0;
#pragma unroll
  for (int i = 1; i < M; ++i) q += v >= (unsigned long long)thr * i ? 1u : 0u;
  return q;
}

// The Pauli frame (fa, fb) of layer l of trajectory tau.
template <int N>
__device__ __forceinline__ void layer_frame(int l, uint32_t tau, const Rng& g, const uint32_t* __restrict__ thr1,
                                            const uint32_t* __restrict__ thr2, int& fa, int& fb) {
  uint32_t a = 0, z = 0, code2[N];
  Philox ph = {{0u, 0u, 0u, 0u}};
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const uint32_t s0 = (uint32_t)(l * N + q) * 2u;   // k = 0; k = 1 is s0 + 1, in the same Philox block
    if (q == 0 || (s0 & 3u) == 0u) ph = philox4x32_10(0x80000000u | (tau << 10) | (s0 >> 2), g.b, g.c_lo, g.c_hi, g.k0, g.k1);
    const uint32_t r0 = (s0 & 2u) ? ph.c[2] : ph.c[0], r1 = (s0 & 2u) ? ph.c[3] : ph.c[1];
    const uint32_t t1 = thr1[q], t2 = thr2[q];
    const uint32_t c0 = r0 < t1 ? 1u + scaled_code<3>(r0, t1) : 0u;
    code2[q] = r1 < t2 ? 1u + scaled_code<15>(r1, t2) : 0u;
    a |= pauli_x(c0) << q;
    z |= pauli_z(c0) << q;
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const int t = (c + 1) % N;
    a ^= ((a >> c) & 1u) << t;
    z ^= ((z >> t) & 1u) << c;
    const uint32_t pc = code2[c] >> 2, pt = code2[c] & 3u;
    a ^= (pauli_x(pc) << c) ^ (pauli_x(pt) << t);
    z ^= (pauli_z(pc) << c) ^ (pauli_z(pt) << t);
  }
  fa = (int)a;
  fb = (int)z;
}

// The same frame (a | b << 16), out of line: for a kernel that draws a frame again inside its state builds (inlined at
// every use, the site loop's registers add to the sweeps': qsim_onchip.hip went to scratch from n = 9 up).
template <int N>
__device__ __noinline__ uint32_t frame_again(int m, uint32_t tau, Rng g, const uint32_t* __restrict__ thr1,
                                             const uint32_t* __restrict__ thr2) {
  int fa, fb;
  layer_frame<N>(m, tau, g, thr1, thr2, fa, fb);
  return (uint32_t)fa | ((uint32_t)fb << 16);
}

// The four shots of Philox block j (shots 4 j .. 4 j + 3) of an `active` lane: outcome from the CDF, the frame's X
// mask, readout flips, then the wave's bit counts into acc.  Every lane of the wave calls it.
template <int N>
__device__ __forceinline__ void draw_block(const uint32_t* cdf, uint32_t tot, uint32_t j, bool active, int shots,
                                           uint32_t amask, bool readout, const uint32_t* __restrict__ thr_ro,
                                           const Rng& g, uint32_t (&acc)[N]) {
  constexpr int D = 1 << N;
  Philox ph = {{0u, 0u, 0u, 0u}};
  if (active) ph = philox4x32_10(j, g.b, g.c_lo, g.c_hi, g.k0, g.k1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t s = 4u * j + r;
    const bool valid = active && s < (uint32_t)shots;
    const uint32_t t = __umulhi(ph.c[r], tot);
    int k = 0;
#pragma unroll
    for (int step = D >> 1; step >= 1; step >>= 1)
      if (cdf[cdf_at(k + step - 1)] <= t) k += step;
    k ^= (int)amask;
    if (readout && valid) {
#pragma unroll
      for (int h = 0; h < (N + 7) / 8; ++h) {
        const Philox pr = philox4x32_10(0x40000000u | (s << 1) | (uint32_t)h, g.b, g.c_lo, g.c_hi, g.k0, g.k1);
        int flip = 0;
#pragma unroll
        for (int i = 8 * h; i < N && i < 8 * h + 8; ++i) {
          const uint32_t field = (pr.c[(i & 7) >> 1] >> (16 * (i & 1))) & 0xFFFFu;
          const uint32_t t01 = thr_ro[2 * i], t10 = thr_ro[2 * i + 1];
          flip |= (field < (((k >> i) & 1) ? t10 : t01) ? 1 : 0) << i;
        }
        k ^= flip;
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += (uint32_t)__popcll(__ballot(valid && ((k >> i) & 1)));
  }
}

// A pass's wave-uniform bit counts into the wave's own row of wcnt (only lane 0 of that wave ever touches the row, so
// no barrier is needed until the rows are summed); the counts then start again from zero.
template <int N>
__device__ __forceinline__ void flush_counts(uint32_t* wcnt, uint32_t (&acc)[N]) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) wcnt[(threadIdx.x >> 6) * N + i] += acc[i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0;
}
// Thread i < N: bit i's count, the four waves' rows added to c1 (after a barrier behind the last flush).
template <int N>
__device__ __forceinline__ int fold_counts(const uint32_t* wcnt, int c1 = 0) {
#pragma unroll
  for (int k = 0; k < NW; ++k) c1 += (int)wcnt[k * N + threadIdx.x];
  return c1;
}

// The state in A -> fp32 probabilities (to probs when non-null) -> quantised words over the state -> scanned CDF.
template <int N>
__device__ __forceinline__ uint32_t state_to_cdf(cf* A, uint32_t* wtot, float* __restrict__ probs) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;
  uint32_t* cdf = reinterpret_cast<uint32_t*>(A);
  uint32_t q[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = threadIdx.x + i * NT;
    if (k < D) {
      const float p = prob_of(A[k]);
      if (probs != nullptr) probs[k] = p;
      q[i] = quantise(p);
    }
  }
  __syncthreads();   // every amplitude has been read: the CDF may overwrite the state
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = threadIdx.x + i * NT;
    if (k < D) cdf[cdf_at(k)] = q[i];
  }
  return cdf_scan<N>(cdf, wtot);
}

// ---- host side of the entry points
// What every noisy entry point requires of its arguments (else hipErrorInvalidValue).
static inline bool noisy_args_ok(int n, int B, int L, int wgroup, int T, const void* thr1, const void* thr2,
                                 const void* thr_ro) {
  if (n < 2 || n > kMaxQubits || B < 1 || L < 1 || 2ll * n * L > kMaxSites) return false;
  if (T < 1 || T > kMaxTraj) return false;
  if (wgroup > 0 && B % wgroup != 0) return false;
  return thr1 != nullptr && thr2 != nullptr && thr_ro != nullptr;
}
// ... and of its shots (T in range): equal shares for the trajectories, whole Philox blocks when there are several.
static inline bool noisy_shots_ok(int shots, int T) {
  if (shots < 1 || shots > kMaxShots || shots % T != 0) return false;
  return T == 1 || (shots / T) % 4 == 0;
}

// The chunks per sample of the kernels that split a sample's trajectories over workgroups.  n >= 10, where the
// registers allow several workgroups per CU and a workgroup lives long (a sample's rebuild count varies, and few long
// workgroups drain badly): the most of 8, 4, 2 that divide T and leave a chunk at least 4 trajectories (measured on
// qsim_noise.hip at B = 2304, n = 12, T = 16 at 1e-3 / 1e-2 gate error: 747 us against 860 us with one workgroup per
// sample).  Below that one workgroup per sample: at n = 8, T = 64 the split gained nothing (342 us against 346 us) and
// its two extra launches cost 3.5 us at zero thresholds (profiles/noise_timing.txt).
static inline int choose_split(int T, int n) {
  if (n < 10) return 1;
  for (int s = 8; s > 1; s >>= 1)
    if (T % s == 0 && T / s >= 4) return s;
  return 1;
}

}  // namespace qnoise
}  // namespace qd
