// Finite-shot measurement of the QSC circuit on the streamed simulator (n = 13 .. 16, L >= 2): the sampling contract
// of csrc/hip/qsim_shots.hip for D = 2^n outcomes whose state does not fit one workgroup's LDS.
//
// The probabilities pass of csrc/hip/qsim_stream.hip (pass_b_probs: the forward's last pass B, storing |amp|^2 in
// natural order instead of reducing <Z>) writes probs (B, D) fp32 and the uint32 total of the quantised words of every
// run of 2048 outcomes.  The sampler gives every 4096-outcome block of a sample one 256-thread workgroup, grid
// (2^(n-12), B): from the sample's run totals it knows base (the blocks before it), mine (its own) and T, builds the
// block's CDF in LDS exactly as the n = 12 sampler does (cdf_at, cdf_scan<12>), regenerates every Philox word of the
// call and keeps the shots with base <= t < base + mine: the outcome is the block index above the 12-bit search for
// t - base.  A block without mass leaves at once; an all-zero row is the last block's (outcome D - 1).  Every block
// writes one row of integer partial counts, a small launch adds the <= 16 rows of a sample and forms E: integers
// throughout, so the result is the sequential sampler's bit for bit (csrc/cpu/qsim_cpu.cpp qd_cpu_sample_z_wide).
//
// Workspace of the entry points: [the forward's workspace | probs (the fused path) | run totals | partial rows].
#include "qsim_shots_dev.h"

namespace qd {
namespace qstream {
// csrc/hip/qsim_stream.hip: the forward's passes with the probabilities pass last (runtot nullable)
int probs_passes(const float* x, const float* w, float* probs, uint32_t* runtot, int B, int n, int L, int wgroup,
                 char* ws, hipStream_t st);
}  // namespace qstream

namespace qshots {

constexpr int kStreamMinQubits = 13, kStreamMaxQubits = 16;
constexpr int RUN = 2048;   // outcomes per run total (the probabilities pass's coalesced output runs)

// runtot[s, r] = the sum of the quantised words of outcomes [2048 r, 2048 (r + 1)) of probs[s]: for probabilities
// the caller supplies (the probabilities pass writes them itself).  Grid (D / 2048, B).
__global__ void __launch_bounds__(NT) run_totals_kernel(const float* __restrict__ probs, uint32_t* __restrict__ runtot,
                                                        int D) {
  __shared__ uint32_t wtot[NW];
  const int r = blockIdx.x, s = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* src = probs + (size_t)s * D + (size_t)r * RUN;
  uint32_t v = 0;
#pragma unroll
  for (int u = 0; u < RUN / (4 * NT); ++u) {
    const float4 p = *reinterpret_cast<const float4*>(src + 4 * threadIdx.x + 4 * NT * u);
    v += quantise(p.x) + quantise(p.y) + quantise(p.z) + quantise(p.w);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if (lane == 0) wtot[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) t += wtot[k];
    runtot[(size_t)s * (D / RUN) + r] = t;
  }
}

// One 4096-outcome block of one sample: cpart[(s, block), i] = the call's shots that fall into the block and have
// bit i of the outcome set.  LDS: the n = 12 sampler's (smem_bytes<12>(false)); the wave counts hold 13 words per
// wave (12 bits + the in-block shots).
template <int N>
__global__ void __launch_bounds__(NT) stream_sample_kernel(const float* __restrict__ probs,
                                                           const uint32_t* __restrict__ runtot,
                                                           int* __restrict__ cpart, int shots, unsigned long long seed,
                                                           unsigned long long ctr0,
                                                           const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N, NBLK = 1 << (N - 12), NC = 13;
  static_assert(O_WCNT + NW * NC * 4 <= O_DATA, "the wave counts fit in front of the CDF");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  uint32_t* cdf = reinterpret_cast<uint32_t*>(smem + O_DATA);
  const int blk = blockIdx.x, s = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* out = cpart + ((size_t)s * NBLK + blk) * N;
  // the sample's run totals (uniform addresses): base, mine, T
  uint32_t base = 0, mine = 0, T = 0;
#pragma unroll
  for (int r = 0; r < 2 * NBLK; ++r) {
    const uint32_t v = runtot[(size_t)s * 2 * NBLK + r];
    T += v;
    if ((r >> 1) < blk) base += v;
    if ((r >> 1) == blk) mine += v;
  }
  const bool zero_row = T == 0 && blk == NBLK - 1;   // an all-zero row: every shot is outcome D - 1, the last block's
  if (mine == 0 && !zero_row) {                      // (uniform over the workgroup)
    if (threadIdx.x < N) out[threadIdx.x] = 0;
    return;
  }
  const float* src = probs + (size_t)s * D + ((size_t)blk << 12);
#pragma unroll
  for (int u = 0; u < 4096 / (4 * NT); ++u) {
    const int k = 4 * threadIdx.x + 4 * NT * u;
    const float4 p = *reinterpret_cast<const float4*>(src + k);
    cdf[cdf_at(k)] = quantise(p.x);
    cdf[cdf_at(k + 1)] = quantise(p.y);
    cdf[cdf_at(k + 2)] = quantise(p.z);
    cdf[cdf_at(k + 3)] = quantise(p.w);
  }
  cdf_scan<12>(cdf, wtot);   // (its total is `mine`)
  const unsigned long long ctr = shot_counter(ctr0, counter);
  uint32_t acc[NC];   // wave-uniform; acc[12]: the shots in this block
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0;
  const uint32_t nblk = ((uint32_t)shots + 3u) >> 2;   // Philox blocks: four shots each
  for (uint32_t j0 = 0; j0 < nblk; j0 += NT) {
    const uint32_t j = j0 + threadIdx.x;
    if (j0 + (uint32_t)wv * 64u >= nblk) break;   // wave-uniform: no lane of this wave holds a shot
    const Philox ph = philox4x32_10(j, (uint32_t)s, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = j < nblk && 4u * j + r < (uint32_t)shots;
      const uint32_t tl = __umulhi(ph.c[r], T) - base;   // (unsigned: below base wraps beyond mine)
      const bool in = valid && (zero_row || tl < mine);
      const unsigned long long min_ = __ballot(in);
      if (min_ == 0ull) continue;   // wave-uniform
      int k = 0;   // the smallest k with cum[k] > tl; lanes outside the block search too (k stays below 4096)
#pragma unroll
      for (int step = 2048; step >= 1; step >>= 1)
        if (cdf[cdf_at(k + step - 1)] <= tl) k += step;
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[i] += (uint32_t)__popcll(__ballot(in && ((k >> i) & 1)));
      acc[12] += (uint32_t)__popcll(min_);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) wcnt[wv * NC + i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int i = threadIdx.x, col = i < 12 ? i : 12;
    int c1 = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) c1 += (int)wcnt[k * NC + col];
    if (i >= 12 && !((blk >> (i - 12)) & 1)) c1 = 0;   // wires above the block: the block index's bits
    out[i] = c1;
  }
}

// counts / E of every (sample, wire): the sum of the sample's partial rows in block order
__global__ void __launch_bounds__(NT) stream_counts_kernel(const int* __restrict__ cpart, float* __restrict__ E,
                                                           int* __restrict__ counts, int B, int n, int shots) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= B * n) return;
  const int s = i / n, q = i % n, nblk = 1 << (n - 12);
  int c1 = 0;
  for (int k = 0; k < nblk; ++k) c1 += cpart[((size_t)s * nblk + k) * n + q];
  E[i] = shots_mean(c1, shots);
  if (counts != nullptr) counts[i] = c1;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t probs_bytes(int n, int B) { return (size_t)B * (4ull << n); }
inline size_t runtot_bytes(int n, int B) { return align256((size_t)B * (1ull << (n - 11)) * 4); }
inline size_t cpart_bytes(int n, int B) { return align256((size_t)B * (1ull << (n - 12)) * n * 4); }

template <int N>
static int launch_blocks(const float* probs, const uint32_t* runtot, int* cpart, int B, int shots,
                         unsigned long long seed, unsigned long long ctr0, const unsigned long long* counter,
                         hipStream_t st) {
  hipLaunchKernelGGL(stream_sample_kernel<N>, dim3(1 << (N - 12), B), dim3(NT), smem_bytes<12>(false), st, probs,
                     runtot, cpart, shots, seed, ctr0, counter);
  return (int)hipGetLastError();
}

// probs + run totals -> E / counts (two launches); ws: [run totals | partial rows]
static int sample_from(const float* probs, char* ws, float* E, int* counts, int B, int n, int shots,
                       unsigned long long seed, unsigned long long ctr0, const unsigned long long* counter,
                       hipStream_t st) {
  const uint32_t* runtot = reinterpret_cast<const uint32_t*>(ws);
  int* cpart = reinterpret_cast<int*>(ws + runtot_bytes(n, B));
  int e;
  switch (n) {
    case 13: e = launch_blocks<13>(probs, runtot, cpart, B, shots, seed, ctr0, counter, st); break;
    case 14: e = launch_blocks<14>(probs, runtot, cpart, B, shots, seed, ctr0, counter, st); break;
    case 15: e = launch_blocks<15>(probs, runtot, cpart, B, shots, seed, ctr0, counter, st); break;
    case 16: e = launch_blocks<16>(probs, runtot, cpart, B, shots, seed, ctr0, counter, st); break;
    default: return (int)hipErrorInvalidValue;
  }
  if (e) return e;
  hipLaunchKernelGGL(stream_counts_kernel, dim3((B * n + NT - 1) / NT), dim3(NT), 0, st, cpart, E, counts, B, n, shots);
  return (int)hipGetLastError();
}

}  // namespace qshots
}  // namespace qd

using namespace qd::qshots;

QD_API int qd_qsim_stream_ok(int n, int L);
QD_API long long qd_qsim_stream_workspace(int n, int B, int L, int backward);

static bool stream_n_ok(int n) { return n >= kStreamMinQubits && n <= kStreamMaxQubits; }
static bool stream_shots_ok(int shots) { return shots >= 1 && shots <= kMaxShots; }

// Workspace bytes of qd_qsim_stream_probs: the streamed forward's.  0 outside its range.
QD_API long long qd_qsim_stream_probs_workspace(int n, int B, int L) {
  if (!qd_qsim_stream_ok(n, L) || B < 1) return 0;
  return qd_qsim_stream_workspace(n, B, L, 0);
}

// Workspace bytes of qd_stream_sample_z: the run totals and the partial rows.
QD_API long long qd_stream_sample_z_workspace(int n, int B) {
  if (!stream_n_ok(n) || B < 1) return 0;
  return (long long)(runtot_bytes(n, B) + cpart_bytes(n, B));
}

// Workspace bytes of qd_qsim_stream_shots_fwd: the forward's, the probabilities, the run totals, the partial rows.
QD_API long long qd_qsim_stream_shots_workspace(int n, int B, int L) {
  if (!qd_qsim_stream_ok(n, L) || B < 1) return 0;
  return qd_qsim_stream_workspace(n, B, L, 0) + (long long)probs_bytes(n, B) + qd_stream_sample_z_workspace(n, B);
}

// qd_qsim_probs for n = 13 .. 16, L >= 2: probs (B, 2^n) fp32, natural basis order.
QD_API int qd_qsim_stream_probs(const float* x, const float* w, float* probs, int B, int n, int L, int wgroup, void* ws,
                                void* stream) {
  if (!qd_qsim_stream_ok(n, L) || B < 1 || ws == nullptr) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
  return qd::qstream::probs_passes(x, w, probs, nullptr, B, n, L, wgroup, (char*)ws, (hipStream_t)stream);
}

// qd_sample_z for n = 13 .. 16.  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_stream_sample_z(const float* probs, float* E, int* counts, int B, int n, int shots,
                              unsigned long long seed, unsigned long long ctr0, const void* counter, void* ws,
                              void* stream) {
  if (!stream_n_ok(n) || !stream_shots_ok(shots) || B < 1 || ws == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(run_totals_kernel, dim3(1 << (n - 11), B), dim3(NT), 0, (hipStream_t)stream, probs,
                     reinterpret_cast<uint32_t*>(ws), 1 << n);
  if (int e = (int)hipGetLastError()) return e;
  return sample_from(probs, (char*)ws, E, counts, B, n, shots, seed, ctr0, (const unsigned long long*)counter,
                     (hipStream_t)stream);
}

// qd_qsim_shots_fwd for n = 13 .. 16, L >= 2: the forward's passes, the probabilities pass (with its run totals),
// the block sampler and the count reduction; only E / counts leave the workspace.
QD_API int qd_qsim_stream_shots_fwd(const float* x, const float* w, float* E, int* counts, int B, int n, int L,
                                    int wgroup, int shots, unsigned long long seed, unsigned long long ctr0,
                                    const void* counter, void* ws, void* stream) {
  if (!qd_qsim_stream_ok(n, L) || !stream_shots_ok(shots) || B < 1 || ws == nullptr) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
  char* base = (char*)ws;
  float* probs = reinterpret_cast<float*>(base + qd_qsim_stream_workspace(n, B, L, 0));
  char* sws = reinterpret_cast<char*>(probs) + probs_bytes(n, B);
  if (int e = qd::qstream::probs_passes(x, w, probs, reinterpret_cast<uint32_t*>(sws), B, n, L, wgroup, base,
                                        (hipStream_t)stream))
    return e;
  return sample_from(probs, sws, E, counts, B, n, shots, seed, ctr0, (const unsigned long long*)counter,
                     (hipStream_t)stream);
}
