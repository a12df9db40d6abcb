// Finite-shot measurement of the QSC circuit under a Pauli noise model (n = 2 .. 12): depolarising-style gate errors
// after every fused RZ.RY and every CNOT of the ring, plus classical readout error.  The shots are split over T error
// realisations ("trajectories"); 256-thread workgroups, one per sample or one per (sample, chunk of trajectories).
//
// Every error is a Pauli and the CNOT ring is Clifford, so all errors of one layer collapse into one Pauli frame
// (X mask a, Z mask b) behind that layer's ring: an index XOR and a sign in the ring gather apply_layer already does
// (qsim_shots_dev.h, FRAMED).  The last layer's frame only XORs the measured outcome.  Trajectories whose frames of
// layers 0 .. L-2 are identity share the noiseless state: the workgroup builds that state and its CDF once, draws the
// shots of all of them from it, and rebuilds the state only for the others.
//
// Split grid (nsplit = 2, 4, 8 chunks of T / nsplit trajectories): a sample's rebuild count varies, and a grid of few,
// long workgroups leaves the CUs idle while its last round drains.  Chunk 0 serves the noiseless CDF for ALL of the
// sample's trajectories plus the rebuilds of its own range; chunk c > 0 only the rebuilds of its range (no noiseless
// state, and nothing at all when every gate threshold is 0).  The chunks' counts meet through integer atomics in E's
// own storage (zeroed by a memset node first) and one tiny launch turns them into E / counts: every result is a
// sum of integers, so it does not depend on the split.
//
// Contract (csrc/cpu/qsim_cpu.cpp qd_cpu_noise_sites / qd_cpu_pauli_frames / qd_cpu_sample_z_noisy implement the same,
// sequentially; everything after the fp32 probability is integer):
//   sites   sigma = (l n + q) 2 + k;  k = 0: after wire q's RZ.RY of layer l,  k = 1: after CNOT(q, (q+1) mod n) of
//           layer l;  2 n L <= 4096
//   draw    of trajectory tau, row b: r = word (sigma & 3) of Philox4x32-10(counter (0x80000000 | tau << 10 |
//           sigma >> 2, b, lo32(c), hi32(c)), key (lo32(seed), hi32(seed))), c = ctr0 + (counter ? *counter : 0);
//           an error occurs iff r < thr (thr1[q] for k = 0, thr2[q] for k = 1); its code is 1 + (uint64(r) 3) / thr
//           for k = 0 (1, 2, 3 = X, Y, Z) and 1 + (uint64(r) 15) / thr for k = 1, code = 4 P_control + P_target
//   frame   of layer l, X -> (x, z) = (1, 0), Y -> (1, 1), Z -> (0, 1): a, b start from the k = 0 codes of the
//           layer's wires; then for c = 0 .. n-1 in ring order, t = (c+1) mod n:  a ^= ((a >> c) & 1) << t;
//           b ^= ((b >> t) & 1) << c;  then the (x, z) bits of CNOT c's k = 1 code are XORed in on wires c and t
//   state   after layer l < L-1:  A'[j] = (-1)^popc(b & (j ^ a)) A_ring[j ^ a]  (global phase dropped); the last
//           layer's a is XORed into every outcome of the trajectory, its b has no effect
//   shots   trajectory tau owns shots [tau S, (tau+1) S), S = shots / T; shot s is drawn exactly as in
//           qsim_shots.hip (Philox block (s >> 2, b, c), word s & 3) from the 2^30 fixed-point CDF of its
//           trajectory's state.  T > 1 needs S % 4 == 0, so a Philox block never straddles two trajectories
//   readout (skipped when every threshold is 0) for shot s, wire i: Philox block with counter (0x40000000 | s << 1 |
//           i >> 3, b, lo32(c), hi32(c)); field = (word[(i & 7) >> 1] >> 16 (i & 1)) & 0xFFFF; the bit, taken after
//           the frame XOR, flips iff field < thr_ro[i][bit]  (bit = 0: readout01, bit = 1: readout10)
//   c1, E, counts as in qsim_shots.hip.  With every threshold 0, E and counts are those of qd_qsim_shots_fwd.
#include "qsim_noise_dev.h"

namespace qd {
namespace qnoise {

// (waves_per_eu 4: at n = 12 the state's 32 KiB let four workgroups share a CU, so the registers must too)
// CACHE: the frames of layers 0 .. L-2 of every trajectory are kept in LDS (a | b << 16; T (L - 1) words) for the
// rebuilds; else (they do not fit the budget) a rebuild draws its frames again.
template <int N, bool CACHE>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4)))
    qsim_noisy_shots_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ E,
                            int* __restrict__ counts, int* __restrict__ acc_out, float* __restrict__ probs_out,
                            int* __restrict__ frames_out,
                            const uint32_t* __restrict__ thr1, const uint32_t* __restrict__ thr2,
                            const uint32_t* __restrict__ thr_ro, int L, int wgroup, int shots, int T,
                            unsigned long long seed, unsigned long long ctr0,
                            const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + O_WTOT);
  uint32_t* wcnt = reinterpret_cast<uint32_t*>(smem + O_WCNT);
  cf* A = reinterpret_cast<cf*>(smem + O_DATA);
  const uint32_t* cdf = reinterpret_cast<const uint32_t*>(smem + O_DATA);
  uint16_t* traj = reinterpret_cast<uint16_t*>(smem + O_DATA + sizeof(cf) * D);   // T words
  uint32_t* fcache = reinterpret_cast<uint32_t*>(smem + O_DATA + sizeof(cf) * D + traj_bytes(T));
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int tlo = chunk * (T / (int)gridDim.y), thi = tlo + T / (int)gridDim.y;   // the rebuilds this workgroup owns
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* xs = x + (size_t)b * N;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * 2 * N * L : 0);
  const unsigned long long ctr = shot_counter(ctr0, counter);
  const Rng g = {(uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)};
  const int S = shots / T;

  uint32_t any_gate = 0, any_ro = 0;   // uniform
#pragma unroll
  for (int q = 0; q < N; ++q) {
    any_gate |= thr1[q] | thr2[q];
    any_ro |= thr_ro[2 * q] | thr_ro[2 * q + 1];
  }
  const bool readout = any_ro != 0;
  if (chunk > 0 && !any_gate) return;   // no frame, so no rebuild: chunk 0 serves every shot
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) wcnt[wv * N + i] = 0;
  }

  // ---- the trajectories' frames: one thread per trajectory (chunk 0 needs every trajectory's word)
  for (int tau = (chunk == 0 ? 0 : tlo) + threadIdx.x; tau < (chunk == 0 ? T : thi); tau += NT) {
    uint16_t word = 0;
    for (int l = 0; l < L; ++l) {
      int fa = 0, fb = 0;
      if (any_gate) layer_frame<N>(l, (uint32_t)tau, g, thr1, thr2, fa, fb);
      if (l < L - 1) {
        if (fa | fb) word |= kRebuild;
        if (CACHE) fcache[tau * (L - 1) + l] = (uint32_t)fa | ((uint32_t)fb << 16);
      } else {
        word |= (uint16_t)fa;
      }
      if (frames_out != nullptr && chunk == 0) {
        int* f = frames_out + (((size_t)b * T + tau) * L + l) * 2;
        f[0] = fa;
        f[1] = fb;
      }
    }
    traj[tau] = word;
  }

  // ---- pass -1: the noiseless state and its CDF, once, and the shots of every trajectory that lives on it;
  //      pass tau >= 0: a trajectory with a frame before the last layer -- the state again, its frames in the ring
  //      gathers, and its own shots
  uint32_t acc[N];   // wave-uniform
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0;
  int pass = -1, base = tlo - 64;
  unsigned long long pending = 0;   // the rebuild flags of trajectories base .. base + 63 not yet served (block-uniform)
  bool first = chunk == 0;          // chunk 0 starts with pass -1
  if (!first) __syncthreads();      // (publishes traj / fcache, as build_state's barriers do for chunk 0)
  for (;;) {
    if (!first) {   // the next trajectory of the range that rebuilds: 64 flags per LDS read
      while (pending == 0ull) {
        base += 64;
        if (base >= thi) break;
        pending = __ballot(base + lane < thi && (traj[base + lane] & kRebuild));
      }
      if (pending == 0ull) break;
      pass = base + __ffsll(pending) - 1;
      pending &= pending - 1ull;
    }
    first = false;
    uint32_t amask_pass = 0;
    if (pass < 0) {
      // Out of line, as qsim_shots.hip's kernels reach it: the function is then compiled on its own in both files,
      // and with zero thresholds the probabilities -- so E and counts -- are those of qd_qsim_shots_fwd bit for bit.
      // Its barriers also publish traj.
      [[clang::noinline]] build_state<N>(A, trig, xs, wsmp, L);
      if (probs_out != nullptr) {
        for (int tau = 0; tau < T; ++tau) {
          if (traj[tau] & kRebuild) continue;
          float* p = probs_out + ((size_t)b * T + tau) * D;
          for (int k = threadIdx.x; k < D; k += NT) p[k] = prob_of(A[k]);
        }
      }
    } else {
      amask_pass = traj[pass] & (kRebuild - 1);
      __syncthreads();   // the previous CDF has been sampled by every wave
      for (int l = 0; l < L; ++l) {
        int fa = 0, fb = 0;
        if (l < L - 1) {
          if (CACHE) {
            const uint32_t f = fcache[pass * (L - 1) + l];
            fa = (int)(f & 0xFFFFu);
            fb = (int)(f >> 16);
          } else {
            layer_frame<N>(l, (uint32_t)pass, g, thr1, thr2, fa, fb);
          }
        }
        layer_trig(trig, wsmp + 2 * N * l, l == 0 ? xs : nullptr, N);
        __syncthreads();
        if (l == 0)
          product_state<N, true>(A, trig, fa, fb);
        else
          apply_layer<N, 3, 0, true>(A, A, trig, fa, fb);
      }
    }
    const uint32_t tot = state_to_cdf<N>(
        A, wtot, pass >= 0 && probs_out != nullptr ? probs_out + ((size_t)b * T + pass) * D : nullptr);
    const uint32_t jlo = pass < 0 ? 0u : ((uint32_t)pass * (uint32_t)S) >> 2;
    const uint32_t jhi = pass < 0 ? ((uint32_t)shots + 3u) >> 2 : ((uint32_t)(pass + 1) * (uint32_t)S + 3u) >> 2;
    for (uint32_t j0 = jlo; j0 < jhi; j0 += NT) {
      const uint32_t j = j0 + threadIdx.x;
      bool active = j < jhi;
      uint32_t amask = amask_pass;
      if (pass < 0 && active) {
        const uint16_t word = traj[(4u * j) / (uint32_t)S];
        active = !(word & kRebuild);
        amask = word & (kRebuild - 1);
      }
      if (__ballot(active) == 0ull) continue;   // wave-uniform
      draw_block<N>(cdf, tot, j, active, shots, amask, readout, thr_ro, g, acc);
    }
    flush_counts<N>(wcnt, acc);
  }

  // ---- counts of the four waves -> E / counts
  __syncthreads();
  if (threadIdx.x < N) {
    const int c1 = fold_counts<N>(wcnt);
    if (acc_out != nullptr) {   // split grid: the chunks' counts meet here
      if (c1 != 0) atomicAdd(acc_out + (size_t)b * N + threadIdx.x, c1);
    } else {
      E[(size_t)b * N + threadIdx.x] = shots_mean(c1, shots);
      if (counts != nullptr) counts[(size_t)b * N + threadIdx.x] = c1;
    }
  }
}

// Split grid: the summed counts (in E's storage) -> counts and E.
__global__ void noisy_finalize_kernel(float* E, int* __restrict__ counts, int total, int shots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c1 = reinterpret_cast<const int*>(E)[i];
  if (counts != nullptr) counts[i] = c1;
  E[i] = shots_mean(c1, shots);
}

static int g_force_split = 0;   // 0: choose; else the number of chunks to launch (tests, timing)

template <int N>
static int launch_noisy(const float* x, const float* w, float* E, int* counts, float* probs_out, int* frames_out,
                        const uint32_t* thr1, const uint32_t* thr2, const uint32_t* thr_ro, int B, int L, int wgroup,
                        int shots, int T, int nsplit, unsigned long long seed, unsigned long long ctr0,
                        const unsigned long long* counter, hipStream_t st) {
  size_t sm = smem_bytes<N>(true) + traj_bytes(T);
  const size_t fc = sizeof(uint32_t) * (size_t)T * (size_t)(L - 1);
  int* acc = nullptr;
  if (nsplit > 1) {
    acc = reinterpret_cast<int*>(E);
    if (hipError_t e = hipMemsetAsync(E, 0, sizeof(float) * (size_t)B * N, st)) return (int)e;
  }
  const dim3 grid(B, nsplit);
  if (sm + fc <= (size_t)kLdsBudget) {
    sm += fc;
    if (hipError_t e = allow_lds(qsim_noisy_shots_kernel<N, true>, sm)) return (int)e;
    hipLaunchKernelGGL((qsim_noisy_shots_kernel<N, true>), grid, dim3(NT), sm, st, x, w, E, counts, acc, probs_out,
                       frames_out, thr1, thr2, thr_ro, L, wgroup, shots, T, seed, ctr0, counter);
  } else {
    if (hipError_t e = allow_lds(qsim_noisy_shots_kernel<N, false>, sm)) return (int)e;
    hipLaunchKernelGGL((qsim_noisy_shots_kernel<N, false>), grid, dim3(NT), sm, st, x, w, E, counts, acc, probs_out,
                       frames_out, thr1, thr2, thr_ro, L, wgroup, shots, T, seed, ctr0, counter);
  }
  if (hipError_t e = hipGetLastError()) return (int)e;
  if (nsplit > 1) {
    const int total = B * N;
    hipLaunchKernelGGL(noisy_finalize_kernel, dim3((total + 255) / 256), dim3(256), 0, st, E, counts, total, shots);
  }
  return (int)hipGetLastError();
}

}  // namespace qnoise
}  // namespace qd

using namespace qd::qnoise;

// E (B, n) fp32 and counts (B, n) int32 (nullable) of `shots` noisy shots per sample, split over T trajectories.
// probs_out (nullable; B, T, 2^n) fp32: the probabilities each trajectory's CDF was quantised from; frames_out
// (nullable; B, T, L, 2) int32: every layer's (a, b).  thr1 / thr2 (n) uint32 gate thresholds, thr_ro (n, 2) uint32
// readout thresholds (<= 65535).  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_qsim_noisy_shots_fwd(const float* x, const float* w, float* E, int* counts, float* probs_out,
                                   int* frames_out, const void* thr1, const void* thr2, const void* thr_ro, int B,
                                   int n, int L, int wgroup, int shots, int T, unsigned long long seed,
                                   unsigned long long ctr0, const void* counter, void* stream) {
  if (!noisy_args_ok(n, B, L, wgroup, T, thr1, thr2, thr_ro) || !noisy_shots_ok(shots, T))
    return (int)hipErrorInvalidValue;
  const int nsplit = g_force_split > 0 ? g_force_split : choose_split(T, n);
  if (T % nsplit != 0) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return launch_noisy<N>(x, w, E, counts, probs_out, frames_out, (const uint32_t*)thr1, (const uint32_t*)thr2,
                           (const uint32_t*)thr_ro, B, L, wgroup, shots, T, nsplit, seed, ctr0,
                           (const unsigned long long*)counter, (hipStream_t)stream);
  });
}

// Tests and timing: launch nsplit (1, 2, 4, 8) chunks per sample from now on; 0 = choose again.  A forced split that
// does not divide T makes qd_qsim_noisy_shots_fwd return hipErrorInvalidValue.
QD_API int qd_qsim_noise_force_split(int nsplit) {
  if (nsplit != 0 && nsplit != 1 && nsplit != 2 && nsplit != 4 && nsplit != 8) return (int)hipErrorInvalidValue;
  g_force_split = nsplit;
  return 0;
}

// The chunks per sample qd_qsim_noisy_shots_fwd launches for T trajectories of n qubits when nothing is forced.
QD_API int qd_qsim_noise_split(int T, int n) { return T >= 1 ? choose_split(T, n) : 0; }
