// On-chip gradients of the QSC circuit (n = 2 .. 12): the parameter-shift rule measured with finite shots on the noisy
// device of qsim_noise.hip.  No new sampling rule: circuit (p, s) of a call with call counter c = ctr0 + *counter is
// measured exactly as qd_qsim_noisy_shots_fwd would measure the circuit, with three substitutions:
//   angle    p = (l n + q) 2 + k is shifted by +pi/2 (s = 0) or -pi/2 (s = 1), as in qsim_pshift.hip;
//   counter  c' = c + ((1 + 2 p + s) << 48) (mod 2^64), qsim_pshift.hip's stream id of the circuit;
//   draws    c' replaces c in all three draw families of qsim_noise.hip: error sites, outcome shots, readout fields.
// Sites, frames, the trajectories' ownership of shots (S = shots / T, S % 4 == 0 for T > 1), thresholds, c1 and E are
// those of qsim_noise.hip / qsim_shots.hip.  Every circuit so has its own error realisations, as on a device; the
// forward keeps id 0.  G[b, p] = sum_j gE[b, j] (E+_j - E-_j) / 2, dx[b, q] = G[b, 2 q], dw = sum_b G[b, :]
// (qd_reduce_slab), as in qsim_pshift.hip; mask and need_dx have its semantics too.
//
// Host composition: circuit (p, s) is sample_z_noisy(qsim_probs(x, w_shifted, frames = F), F[..., L-1, 0], noise,
// shots, seed, c') with F = pauli_frames(noise_sites(noise, B, n, L, T, seed, c')).  With every threshold zero Epm and
// G are those of qd_qsim_pshift at the same shots: the noiseless shifted state is qsim_pshift_dev.h's shifted_state in
// both kernels, the same inline pieces in the same order, and everything behind the fp32 probability is integer.
//
// Grid as in qd_qsim_pshift: one 256-thread workgroup per (sample, layer l, chunk of the layer's qubits); the state
// that enters layer l is built once and kept (second LDS buffer, registers at n = 12).  Per circuit: one thread per
// trajectory draws the frames under c' (traj word and, when it fits, the frames of layers 0 .. L-2 in LDS); the shifted
// noiseless state and its CDF serve every trajectory whose frames before the last layer are identity (skipped when
// there is none); a trajectory with a frame only at or after layer l restarts from the kept state, layers l .. L-1
// with the frames in the ring gathers; one with a frame before layer l is built from the product state.  The last
// layer's RZ shifts change no probability: one noiseless state and CDF serve all such circuits of the workgroup
// (their counts parked in LDS), then each circuit's rebuilding trajectories follow under its own c'.
#include <algorithm>

#include "qsim_noise_dev.h"
#include "qsim_pshift_dev.h"

namespace qd {
namespace qonchip {
using namespace qd::qshots;
using namespace qd::qnoise;
using namespace qd::qpshift;

// LDS carve (bytes): qsim_shots.hip's (trig | scan totals | per-wave bit counts) | gE of the sample | E+ and E- of the
// parameter at hand | the parked counts of the last layer's RZ circuits (<= 2 x 12 circuits x 12 words) | the working
// state, later its CDF | (n <= 11) the state that enters the layer | traj words (T) | (CACHE) frames (T (L - 1))
constexpr int O_GE = 512, O_EPM = 576, O_PARK = 768, O_STATE = 1920;
constexpr uint16_t kEarly = 0x4000;      // traj word: a frame before the workgroup's layer l is not identity
constexpr uint16_t kXMask = 0x0fff;      // traj word: the last layer's X mask
constexpr int kTargetBlocks = 8192;      // as qsim_pshift.hip
template <int N>
constexpr size_t lds_bytes(int T) {
  return O_STATE + (reg_prefix<N>() ? 1 : 2) * sizeof(cf) * (1 << N) + traj_bytes(T);
}
static_assert(lds_bytes<12>(kMaxTraj) <= (size_t)kLdsBudget, "a quarter of a CU's LDS at n = 12");
static_assert(lds_bytes<11>(kMaxTraj) <= (size_t)kLdsBudget, "a quarter of a CU's LDS at n = 11");

// (waves_per_eu: at n = 12 the kept state's 64 registers must leave three workgroups per CU, 168 VGPRs.  The cap
// costs 46 spilled dwords; uncapped, 198 VGPRs and two workgroups per CU measured 2027 against 1581 us at zero
// thresholds and 13595 against 10350 us at the noise point, B = 256, L = 3, 1024 shots, T = 16:
// profiles/onchip_timing.txt)
#ifndef QD_ONCHIP_WAVES12
#define QD_ONCHIP_WAVES12 3
#endif
template <int N, bool CACHE>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(N >= 12 ? QD_ONCHIP_WAVES12 : 1)))
    qsim_onchip_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ gE,
                       float* __restrict__ G, float* __restrict__ Epm, float* __restrict__ probs,
                       int* __restrict__ frames_out, const unsigned char* __restrict__ mask,
                       const uint32_t* __restrict__ thr1, const uint32_t* __restrict__ thr2,
                       const uint32_t* __restrict__ thr_ro, int L, int wgroup, int chunks, int need_dx, int shots, int T,
                       unsigned long long seed, unsigned long long ctr0,
                       const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;
  constexpr int GB = group_bits<N>();
  constexpr bool RP = reg_prefix<N>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  float* ges = reinterpret_cast<float*>(smem + O_GE);
  float* epm = reinterpret_cast<float*>(smem + O_EPM);
  uint32_t* park = reinterpret_cast<uint32_t*>(smem + O_PARK);
  cf* A = reinterpret_cast<cf*>(smem + O_STATE);
  uint32_t* cdf = reinterpret_cast<uint32_t*>(smem + O_STATE);   // over the working state, once it has been read
  cf* Pfx = RP ? A : A + D;
  uint16_t* traj = reinterpret_cast<uint16_t*>(smem + O_STATE + (RP ? 1 : 2) * sizeof(cf) * D);
  uint32_t* fcache = reinterpret_cast<uint32_t*>(smem + O_STATE + (RP ? 1 : 2) * sizeof(cf) * D + traj_bytes(T));
  const int chunk = blockIdx.x % chunks, l = (blockIdx.x / chunks) % L, b = blockIdx.x / (chunks * L);
  const int q0 = chunk * N / chunks, q1 = (chunk + 1) * N / chunks;   // this workgroup's qubits
  const int P = 2 * N * L;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* xs = x + (size_t)b * N;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * P : 0);
  const bool last = l == L - 1;
  const int S = shots / T;

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

  uint32_t any_gate = 0, any_ro = 0;   // uniform
#pragma unroll
  for (int q = 0; q < N; ++q) {
    any_gate |= thr1[q] | thr2[q];
    any_ro |= thr_ro[2 * q] | thr_ro[2 * q + 1];
  }
  const bool readout = any_ro != 0;

  // the state that enters layer l: in Pfx (LDS), or the thread's share of it in pfx
  cf pfx[RP ? FirstSweep<N>::AMPS : 1];
  if (l > 0) {
    prefix_state<N>(Pfx, trig, wsmp, xs, l);
    if constexpr (RP) keep_state<N>(pfx, A);   // (a thread rewrites these amplitudes of A itself, in first_sweep)
  }

  auto rng_of = [&](int p, int s) -> Rng {
    const unsigned long long id = 1ull + 2ull * (unsigned long long)p + (unsigned long long)s;
    const unsigned long long cc = ctr + (id << 48);
    return Rng{(uint32_t)b, (uint32_t)cc, (uint32_t)(cc >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)};
  };
  size_t slot = 0;   // circuit (p, s) of sample b in Epm / probs / frames
  auto circuit_slot = [&](int p, int s) { slot = ((size_t)b * P + p) * 2 + s; };

  uint32_t acc[N];   // wave-uniform bit counts of the pass at hand
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0;
  // a circuit's counts start from zero (a wave's row of wcnt is written by its lane 0 alone; the rows were last read
  // before the barrier that ended the previous circuit)
  auto zero_counts = [&]() {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i) wcnt[wv * N + i] = 0;
    }
  };

  // The circuit's frames under its counter: one thread per trajectory, integer only.  Ends with a barrier; returns
  // whether any trajectory lives on the noiseless state (block-uniform).
  auto draw_frames = [&](const Rng& g, bool write) -> bool {
    int plain = 0;
    for (int tau = threadIdx.x; tau < T; tau += NT) {
      uint16_t word = 0;
      for (int m = 0; m < L; ++m) {
        int fa = 0, fb = 0;
        if (any_gate) layer_frame<N>(m, (uint32_t)tau, g, thr1, thr2, fa, fb);
        if (m < L - 1) {
          if (fa | fb) word |= (uint16_t)(kRebuild | (m < l ? kEarly : 0));
          if (CACHE) fcache[tau * (L - 1) + m] = (uint32_t)fa | ((uint32_t)fb << 16);
        } else {
          word |= (uint16_t)fa;
        }
        if (frames_out != nullptr && write) {
          int* f = frames_out + (((slot * T + tau) * L) + m) * 2;
          f[0] = fa;
          f[1] = fb;
        }
      }
      traj[tau] = word;
      plain |= !(word & kRebuild);
    }
    return __syncthreads_or(plain) != 0;
  };

  float pr[PER];   // the probabilities of the noiseless state in A, outcome threadIdx.x + i NT
  auto read_probs = [&]() {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) pr[i] = prob_of(A[k]);
    }
  };
  // pr into the probs slot of every trajectory that lives on the noiseless state
  auto store_plain_probs = [&]() {
    if (probs == nullptr) return;
    for (int tau = 0; tau < T; ++tau) {
      if (traj[tau] & kRebuild) continue;
      float* dst = probs + (slot * T + tau) * D;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int k = threadIdx.x + i * NT;
        if (k < D) dst[k] = pr[i];
      }
    }
  };
  // quantised pr -> CDF over the state; returns the total
  auto make_cdf = [&]() -> uint32_t {
    __syncthreads();   // every amplitude has been read: the CDF may overwrite the state
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = threadIdx.x + i * NT;
      if (k < D) cdf[cdf_at(k)] = quantise(pr[i]);
    }
    return cdf_scan<N>(cdf, wtot);
  };
  // the shots of every trajectory that lives on the noiseless CDF, into the waves' counts
  auto serve_plain = [&](uint32_t tot, const Rng& g) {
    const uint32_t jhi = ((uint32_t)shots + 3u) >> 2;
    for (uint32_t j0 = 0; j0 < jhi; j0 += NT) {
      const uint32_t j = j0 + threadIdx.x;
      bool active = j < jhi;
      uint32_t amask = 0;
      if (active) {
        const uint16_t word = traj[(4u * j) / (uint32_t)S];
        active = !(word & kRebuild);
        amask = word & kXMask;
      }
      if (__ballot(active) == 0ull) continue;   // wave-uniform
      draw_block<N>(cdf, tot, j, active, shots, amask, readout, thr_ro, g, acc);
    }
    flush_counts<N>(wcnt, acc);
  };
  // the frame (fa, fb) behind layer m of trajectory tau, for the state build (the last layer's acts on the outcome)
  auto frame_of = [&](int tau, int m, const Rng& g, int& fa, int& fb) {
    fa = 0;
    fb = 0;
    if (m >= L - 1) return;
    const uint32_t f = CACHE ? fcache[tau * (L - 1) + m] : frame_again<N>(m, (uint32_t)tau, g, thr1, thr2);
    fa = (int)(f & 0xFFFFu);
    fb = (int)(f >> 16);
  };
  // every trajectory of the circuit that rebuilds: its state with the frames in the ring gathers (layer l's angle
  // (sq, sk) shifted by sh), its CDF and its own shots
  auto rebuilds = [&](const Rng& g, int sq, int sk, float sh) {
    int base = -64;
    unsigned long long pending = 0;   // the rebuild flags of trajectories base .. base + 63 not yet served (uniform)
    for (;;) {
      while (pending == 0ull) {
        base += 64;
        if (base >= T) break;
        pending = __ballot(base + lane < T && (traj[base + lane] & kRebuild));
      }
      if (pending == 0ull) break;
      const int tau = base + __ffsll((long long)pending) - 1;
      pending &= pending - 1ull;
      const uint16_t word = traj[tau];
      __syncthreads();   // the previous CDF has been sampled by every wave
      int fa, fb;
      if (l == 0 || (word & kEarly)) {   // from the product state, every frame
        for (int m = 0; m < L; ++m) {
          frame_of(tau, m, g, fa, fb);
          layer_trig_shifted(trig, wsmp + 2 * N * m, m == 0 ? xs : nullptr, N, m == l ? sq : -1, sk, sh);
          __syncthreads();
          if (m == 0)
            product_state<N, true>(A, trig, fa, fb);
          else
            apply_layer<N, GB, 0, true>(A, A, trig, fa, fb);
        }
      } else {   // from the kept state: layers l .. L-1
        frame_of(tau, l, g, fa, fb);
        layer_trig_shifted(trig, wsmp + 2 * N * l, nullptr, N, sq, sk, sh);
        __syncthreads();
        if constexpr (RP) {
          first_sweep<N>(pfx, A, trig);
          apply_layer<N, GB, 1, true>(A, A, trig, fa, fb);
        } else {
          apply_layer<N, GB, 0, true>(Pfx, A, trig, fa, fb);
        }
        for (int m = l + 1; m < L; ++m) {
          frame_of(tau, m, g, fa, fb);
          layer_trig(trig, wsmp + 2 * N * m, nullptr, N);
          __syncthreads();
          apply_layer<N, GB, 0, true>(A, A, trig, fa, fb);
        }
      }
      const uint32_t tot = state_to_cdf<N>(A, wtot, probs != nullptr ? probs + (slot * T + tau) * D : nullptr);
      const uint32_t jlo = ((uint32_t)tau * (uint32_t)S) >> 2;
      const uint32_t jhi = ((uint32_t)(tau + 1) * (uint32_t)S + 3u) >> 2;
      for (uint32_t j0 = jlo; j0 < jhi; j0 += NT) {
        const uint32_t j = j0 + threadIdx.x;
        const bool active = j < jhi;
        if (__ballot(active) == 0ull) continue;   // wave-uniform
        draw_block<N>(cdf, tot, j, active, shots, word & kXMask, readout, thr_ro, g, acc);
      }
      flush_counts<N>(wcnt, acc);
    }
  };
  // the waves' counts (plus parked ones) -> E of circuit (p, s), into epm[s] and Epm.  Ends with a barrier.
  auto finish = [&](int s, const uint32_t* parked) {
    __syncthreads();
    if (threadIdx.x < N) {
      const int c1 = fold_counts<N>(wcnt, parked != nullptr ? (int)parked[threadIdx.x] : 0);
      const float e = shots_mean(c1, shots);
      epm[s * N + threadIdx.x] = e;
      if (Epm != nullptr) Epm[slot * N + threadIdx.x] = e;
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
        const float sh = s == 0 ? kHalfPi : -kHalfPi;
        const Rng g = rng_of(p, s);
        circuit_slot(p, s);
        zero_counts();
        if (draw_frames(g, true)) {
          shifted_state<N>(A, Pfx, pfx, trig, wsmp, xs, l, L, q, k, sh);
          read_probs();
          store_plain_probs();
          const uint32_t tot = make_cdf();
          serve_plain(tot, g);
        }
        if (any_gate) rebuilds(g, q, k, sh);
        finish(s, nullptr);
      }
      store_G(p);
    }
  }
  if (!last) return;
  // the last layer's RZ shifts: phases only, every circuit has the unshifted circuit's probabilities.  First every
  // circuit's trajectories that live on the one noiseless CDF, their counts parked; then, the CDF given up, every
  // circuit's rebuilds (its frames drawn again).
  bool any_rz = false;
  for (int q = q0; q < q1; ++q) any_rz = any_rz || runs(q, 1);
  if (!any_rz) return;
  shifted_state<N>(A, Pfx, pfx, trig, wsmp, xs, l, L, -1, 0, 0.f);
  read_probs();
  const uint32_t tot = make_cdf();
  int ci = 0;
  for (int q = q0; q < q1; ++q) {
    if (!runs(q, 1)) continue;
    const int p = (l * N + q) * 2 + 1;
    for (int s = 0; s < 2; ++s, ++ci) {
      const Rng g = rng_of(p, s);
      circuit_slot(p, s);
      zero_counts();
      draw_frames(g, true);
      store_plain_probs();
      serve_plain(tot, g);
      __syncthreads();
      if (threadIdx.x < N) park[ci * N + threadIdx.x] = (uint32_t)fold_counts<N>(wcnt);
      __syncthreads();
    }
  }
  ci = 0;
  for (int q = q0; q < q1; ++q) {
    if (!runs(q, 1)) continue;
    const int p = (l * N + q) * 2 + 1;
    for (int s = 0; s < 2; ++s, ++ci) {
      const Rng g = rng_of(p, s);
      circuit_slot(p, s);
      zero_counts();
      if (any_gate) {
        draw_frames(g, false);
        rebuilds(g, -1, 0, 0.f);
      }
      finish(s, park + ci * N);
    }
    store_G(p);
  }
}

template <int N>
static int launch(const float* x, const float* w, const float* gE, float* G, float* Epm, float* probs, int* frames_out,
                  const unsigned char* mask, const uint32_t* thr1, const uint32_t* thr2, const uint32_t* thr_ro, int B,
                  int L, int wgroup, int need_dx, int shots, int T, unsigned long long seed, unsigned long long ctr0,
                  const unsigned long long* counter, hipStream_t st) {
  size_t sm = lds_bytes<N>(T);
  const size_t fc = sizeof(uint32_t) * (size_t)T * (size_t)(L - 1);
  const long long bl = (long long)B * L;
  int chunks = (int)std::min<long long>(N, std::max<long long>(1, (kTargetBlocks + bl - 1) / bl));
  while (N % chunks != 0) ++chunks;   // equal shares of the qubits
  const dim3 grid((unsigned)(bl * chunks));
  if (sm + fc <= (size_t)kLdsBudget) {
    sm += fc;
    if (hipError_t e = allow_lds(qsim_onchip_kernel<N, true>, sm)) return (int)e;
    hipLaunchKernelGGL((qsim_onchip_kernel<N, true>), grid, dim3(NT), sm, st, x, w, gE, G, Epm, probs, frames_out, mask,
                       thr1, thr2, thr_ro, L, wgroup, chunks, need_dx, shots, T, seed, ctr0, counter);
  } else {
    if (hipError_t e = allow_lds(qsim_onchip_kernel<N, false>, sm)) return (int)e;
    hipLaunchKernelGGL((qsim_onchip_kernel<N, false>), grid, dim3(NT), sm, st, x, w, gE, G, Epm, probs, frames_out,
                       mask, thr1, thr2, thr_ro, L, wgroup, chunks, need_dx, shots, T, seed, ctr0, counter);
  }
  return (int)hipGetLastError();
}

}  // namespace qonchip
}  // namespace qd

// G (B, P) fp32 of the 2 P shifted circuits of every sample, each measured with `shots` noisy shots over T
// trajectories; Epm (nullable; B, P, 2, n) fp32, probs (nullable; B, P, 2, T, 2^n) fp32 the probabilities each
// trajectory's CDF was quantised from, frames_out (nullable; B, P, 2, T, L, 2) int32.  x (B, n), w (L, n, 2) or grouped
// (wgroup samples per group), gE (B, n), mask (nullable; P) uint8; thr1 / thr2 (n) uint32 gate thresholds, thr_ro
// (n, 2) uint32 readout thresholds (<= 65535).  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_qsim_noisy_pshift(const float* x, const float* w, const float* gE, float* G, float* Epm, float* probs,
                                int* frames_out, const unsigned char* mask, const void* thr1, const void* thr2,
                                const void* thr_ro, int B, int n, int L, int wgroup, int need_dx, int shots, int T,
                                unsigned long long seed, unsigned long long ctr0, const void* counter, void* stream) {
  using namespace qd::qnoise;
  if (!noisy_args_ok(n, B, L, wgroup, T, thr1, thr2, thr_ro) || !noisy_shots_ok(shots, T))
    return (int)hipErrorInvalidValue;
  if (4ll * n * L + 1 >= (1ll << 16)) return (int)hipErrorInvalidValue;   // stream ids 0 .. 2 P fit 16 bits
  if ((long long)B * L * n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return qd::qonchip::launch<N>(x, w, gE, G, Epm, probs, frames_out, mask, (const uint32_t*)thr1,
                                  (const uint32_t*)thr2, (const uint32_t*)thr_ro, B, L, wgroup, need_dx, shots, T, seed,
                                  ctr0, (const unsigned long long*)counter, (hipStream_t)stream);
  });
}
