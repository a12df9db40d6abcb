// Parameter-shift gradients of the QSC circuit (n = 2 .. 12), exact or finite-shot: the gradient an on-chip QNN can
// measure.  Parameter p = (l n + q) 2 + k is w[l, q, k] (k = 0: the RY angle, 1: the RZ angle), P = 2 n L; circuit
// (p, s) is sample b's circuit with that one angle shifted by +pi/2 (s = 0) or -pi/2 (s = 1), and
//   G[b, p] = sum_j gE[b, j] (E+_j - E-_j) / 2,    E+- = <Z> of the two shifted circuits.
// The layer-0 RY gate is RY(x_q + w[0, q, 0]), so dx[b, q] = G[b, 2 q]; dw = sum_b G[b, :] (qd_reduce_slab).
//
// One 256-thread workgroup per (sample, layer, chunk of the layer's qubits).  The shifted circuits of a layer share
// the state that enters the layer: the workgroup builds it once and keeps it, and only layers l .. L-1 run per
// circuit (layer 0 starts from its product state).  It is kept in a second LDS buffer for n <= 11; at n = 12 two
// states would leave two workgroups per CU, so there every thread keeps in registers the amplitudes it owns in the
// layer's first pair sweep (32 of 160 VGPRs: three workgroups per CU; measured 1518 against 2190 us per launch at
// B = 256, L = 3, 1024 shots -- and the other way round at n = 8, where the registers cost a wave per SIMD).
// A last-layer RZ shift changes no probability: a workgroup's circuits of that kind share one state and one CDF,
// drawn from under their own stream ids; in exact mode their G is exactly 0.  The chunk count trades the shared
// prefix against the machine's fill (small batches of 12 qubits) and the layers' unequal work; the launcher picks it.
//
// shots == 0: E = sum_k p_k z_k of the shifted state.  shots >= 1: that many shots per shifted circuit under the
// sampling contract at the top of qsim_shots.hip (quantisation, CDF, Philox words and outcome search unchanged), with
// the 64-bit call counter c' = c + (id << 48) (mod 2^64), id = 1 + 2 p + s, c = ctr0 + *counter.  The forward keeps
// id 0, so for call counters c < 2^48 no backward stream coincides with a forward's or with another circuit's (above
// that bound an id's streams run into the next id's), and a row's shots do not depend on B.  2 P + 1 < 2^16.
//
// mask (nullable, (P,) uint8): with mask[p] == 0 neither circuit of p runs, G[:, p] = 0 and p's Epm / probs slots are
// left untouched -- except that with need_dx a layer-0 RY parameter's circuits still run (dx comes out of them; the
// caller keeps the masked dw[p] at 0).
#include <algorithm>

#include "qsim_pshift_dev.h"

namespace qd {
namespace qpshift {

// LDS carve (bytes): qsim_shots.hip's (trig | scan totals | per-wave bit counts), then gE of the sample (<= 12
// floats) | E+ and E- of the parameter at hand (2 x 12 floats) | the working state, later its CDF | (n <= 11) the
// state that enters the layer
constexpr int O_GE = 512, O_EPM = 576, O_STATE = 768;
template <int N>
constexpr size_t smem_bytes() {
  return O_STATE + (reg_prefix<N>() ? 1 : 2) * sizeof(cf) * (1 << N);
}

constexpr int kTargetBlocks = 8192;   // workgroups a launch is split towards: some rounds of 256 CUs x 2 .. 8 each

template <int N>
__global__ void __launch_bounds__(NT) qsim_pshift_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ gE, float* __restrict__ G,
                                                         float* __restrict__ Epm, float* __restrict__ probs,
                                                         const unsigned char* __restrict__ mask, int L, int wgroup,
                                                         int chunks, int need_dx, int shots, unsigned long long seed,
                                                         unsigned long long ctr0,
                                                         const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  float* wsum = reinterpret_cast<float*>(smem + O_WCNT);   // exact mode: per-wave partial sums instead of counts
  float* ges = reinterpret_cast<float*>(smem + O_GE);
  float* epm = reinterpret_cast<float*>(smem + O_EPM);
  cf* A = reinterpret_cast<cf*>(smem + O_STATE);
  uint32_t* cdf = reinterpret_cast<uint32_t*>(smem + O_STATE);   // over the working state, once it has been read
  const int chunk = blockIdx.x % chunks, l = (blockIdx.x / chunks) % L, b = blockIdx.x / (chunks * L);
  const int q0 = chunk * N / chunks, q1 = (chunk + 1) * N / chunks;   // this workgroup's qubits
  const int P = 2 * N * L;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* xs = x + (size_t)b * N;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * P : 0);
  const bool last = l == L - 1;

  // which of the layer's parameters run (block-uniform)
  auto runs = [&](int q, int k) -> bool {
    return mask == nullptr || mask[(l * N + q) * 2 + k] != 0 || (need_dx && l == 0 && k == 0);
  };
  bool any = false;
  for (int t = 2 * q0; t < 2 * q1; ++t) any = any || runs(t >> 1, t & 1);
  if (threadIdx.x >= 2 * q0 && threadIdx.x < 2 * q1 && !runs(threadIdx.x >> 1, threadIdx.x & 1))
    G[(size_t)b * P + l * 2 * N + threadIdx.x] = 0.f;
  if (!any) return;
  if (threadIdx.x < N) ges[threadIdx.x] = gE[(size_t)b * N + threadIdx.x];
  const unsigned long long ctr = shot_counter(ctr0, counter);

  // the state that enters layer l: in Pfx (LDS), or the thread's share of it in pfx
  constexpr bool RP = reg_prefix<N>();
  cf* Pfx = RP ? A : A + D;
  cf pfx[RP ? FirstSweep<N>::AMPS : 1];
  if (l > 0) {
    prefix_state<N>(Pfx, trig, wsmp, xs, l);
    if constexpr (RP) keep_state<N>(pfx, A);   // (a thread rewrites these amplitudes of A itself, in first_sweep)
  }

  // the final state, in A, of the circuit with layer l's angle (sq, sk) shifted by sh (sq < 0: the circuit itself)
  auto make_state = [&](int sq, int sk, float sh) { shifted_state<N>(A, Pfx, pfx, trig, wsmp, xs, l, L, sq, sk, sh); };
  float pr[PER];   // the probabilities of the state in A, outcome threadIdx.x + i NT
  auto read_probs = [&]() {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) pr[i] = prob_of(A[k]);
    }
  };
  auto store_probs = [&](int p, int s) {
    if (probs == nullptr) return;
    float* dst = probs + (((size_t)b * P + p) * 2 + s) * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) dst[k] = pr[i];
    }
  };
  // quantised pr -> CDF over the state; returns T
  auto make_cdf = [&]() -> uint32_t {
    __syncthreads();   // every amplitude has been read: the CDF may overwrite the state
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) cdf[cdf_at(k)] = quantise(pr[i]);
    }
    return cdf_scan<N>(cdf, wtot);
  };
  // E of circuit (p, s) into epm[s] and Epm: exact from pr, or `shots` draws from the CDF.  Ends with a barrier.
  auto exact_E = [&](int p, int s) {
    float part[N];
#pragma unroll
    for (int i = 0; i < N; ++i) part[i] = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) {
#pragma unroll
        for (int j = 0; j < N; ++j) part[j] += ((k >> j) & 1) ? -pr[i] : pr[i];
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) part[j] += __shfl_xor(part[j], d);
      if (lane == 0) wsum[wv * N + j] = part[j];
    }
    __syncthreads();
    if (threadIdx.x < N) {
      float e = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) e += wsum[k * N + threadIdx.x];
      epm[s * N + threadIdx.x] = e;
      if (Epm != nullptr) Epm[(((size_t)b * P + p) * 2 + s) * N + threadIdx.x] = e;
    }
    __syncthreads();
  };
  auto sampled_E = [&](uint32_t T, int p, int s) {
    const unsigned long long id = 1ull + 2ull * (unsigned long long)p + (unsigned long long)s;
    const int c1 = shot_counts<N, true>(cdf, T, wcnt, b, shots, seed, ctr + (id << 48));
    if (threadIdx.x < N) {
      const float e = shots_mean(c1, shots);
      epm[s * N + threadIdx.x] = e;
      if (Epm != nullptr) Epm[(((size_t)b * P + p) * 2 + s) * N + threadIdx.x] = e;
    }
    __syncthreads();
  };
  // G[b, p] from epm (after a barrier; epm is next written only behind further barriers)
  auto store_G = [&](int p) {
    if (threadIdx.x == 0) {
      float g = 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) g += ges[j] * (0.5f * (epm[j] - epm[N + j]));
      G[(size_t)b * P + p] = g;
    }
  };

  for (int q = q0; q < q1; ++q) {
    for (int k = 0; k < (last ? 1 : 2); ++k) {
      if (!runs(q, k)) continue;
      const int p = (l * N + q) * 2 + k;
      for (int s = 0; s < 2; ++s) {
        make_state(q, k, s == 0 ? kHalfPi : -kHalfPi);
        read_probs();
        store_probs(p, s);
        if (shots == 0) {
          exact_E(p, s);
        } else {
          const uint32_t T = make_cdf();
          sampled_E(T, p, s);
        }
      }
      store_G(p);
    }
  }
  if (!last) return;
  // the last layer's RZ shifts: phases only, every circuit has the unshifted circuit's probabilities
  bool any_rz = false;
  for (int q = q0; q < q1; ++q) any_rz = any_rz || runs(q, 1);
  if (!any_rz) return;
  make_state(-1, 0, 0.f);
  read_probs();
  uint32_t T = 0;
  if (shots > 0) T = make_cdf();
  for (int q = q0; q < q1; ++q) {
    if (!runs(q, 1)) continue;
    const int p = (l * N + q) * 2 + 1;
    for (int s = 0; s < 2; ++s) {
      store_probs(p, s);
      if (shots == 0)
        exact_E(p, s);
      else
        sampled_E(T, p, s);
    }
    store_G(p);
  }
}

template <int N>
static int launch(const float* x, const float* w, const float* gE, float* G, float* Epm, float* probs,
                  const unsigned char* mask, int B, int L, int wgroup, int need_dx, int shots, unsigned long long seed,
                  unsigned long long ctr0, const unsigned long long* counter, hipStream_t st) {
  const size_t sm = smem_bytes<N>();
  if (hipError_t e = allow_lds(qsim_pshift_kernel<N>, sm)) return (int)e;
  const long long bl = (long long)B * L;
  int chunks = (int)std::min<long long>(N, std::max<long long>(1, (kTargetBlocks + bl - 1) / bl));
  while (N % chunks != 0) ++chunks;   // equal shares of the qubits
  hipLaunchKernelGGL(qsim_pshift_kernel<N>, dim3((unsigned)(bl * chunks)), dim3(NT), sm, st, x, w, gE, G, Epm, probs,
                     mask, L, wgroup, chunks, need_dx, shots, seed, ctr0, counter);
  return (int)hipGetLastError();
}

}  // namespace qpshift
}  // namespace qd

// G (B, P) fp32, Epm (nullable; B, P, 2, n) fp32 and probs (nullable; B, P, 2, 2^n) fp32 of the 2 P shifted circuits
// of every sample; x (B, n), w (L, n, 2) or grouped (wgroup samples per group), gE (B, n), mask (nullable; P) uint8.
// shots = 0: exact expectations.  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_qsim_pshift(const float* x, const float* w, const float* gE, float* G, float* Epm, float* probs,
                          const unsigned char* mask, int B, int n, int L, int wgroup, int need_dx, int shots,
                          unsigned long long seed, unsigned long long ctr0, const void* counter, void* stream) {
  using namespace qd::qshots;
  if (n < 2 || n > kMaxQubits || B < 1 || L < 1 || shots < 0 || shots > kMaxShots) return (int)hipErrorInvalidValue;
  if (4ll * n * L + 1 >= (1ll << 16)) return (int)hipErrorInvalidValue;   // stream ids 0 .. 2 P fit 16 bits
  if ((long long)B * L * n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return qd::qpshift::launch<N>(x, w, gE, G, Epm, probs, mask, B, L, wgroup, need_dx, shots, seed, ctr0,
                                  (const unsigned long long*)counter, (hipStream_t)stream);
  });
}
