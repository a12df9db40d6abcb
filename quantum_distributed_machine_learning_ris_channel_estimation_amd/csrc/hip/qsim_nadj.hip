// Noise-aware adjoint gradients of the QSC circuit (n = 2 .. 12): the adjoint method run through the Pauli frames
// that qsim_noise.hip samples.  A trajectory is a unitary circuit with fixed Paulis behind its rings, so its exact
// gradient costs one forward build and one reverse sweep -- not the 2 P shifted circuits of qsim_onchip.hip.
//
// Contract.  No new sampling rule: for a call with counter c = ctr0 + (counter ? *counter : 0) the frames
// F[b, tau, l] = (a, b) are those qd_qsim_noisy_shots_fwd draws under the same (seed, c, row b, tau) -- layer_frame of
// qsim_noise_dev.h, i.e. pauli_frames(noise_sites(...)) on the host.  With thr_ro[j] = (thr01_j, thr10_j):
//   E_j^tau   exact <Z_j> of trajectory tau's circuit, the frames of layers 0 .. L-2 behind their rings
//   s_j(tau)  -1 when bit j of the last layer's X mask a[L-1] is set, else +1  (its Z mask has no effect)
//   c_j = 1 - (thr01_j + thr10_j) / 65536,  d_j = (thr10_j - thr01_j) / 65536
//   Ebar[b, j] = c_j (1/T) sum_tau s_j(tau) E_j^tau + d_j     (the mean of the noisy shots forward's E given F)
//   G[b, p]    = sum_j gE[b, j] dEbar[b, j] / dtheta_p,  p = (l n + q) 2 + k as in qsim_pshift.hip;
//                dx[b, q] = G[b, 2 q],  dw = sum_b G[b, :]  (qd_reduce_slab)
// Host composition: the parameter-shift rule over qsim_probs(frames=) in fp64 (ops/quantum.py _nadj_rows_cpu).
//
// Passes of a sample.  Every trajectory whose frames before the last layer are identity lives on the noiseless state:
// they take ONE pass together, lambda = (sum_j g'_j Z_j) psi with g'_j = gE_j c_j (sum of their s_j) / T (the sum is
// an integer; the pass is skipped when the set is empty).  Every other trajectory takes a pass of its own with
// g'_j = gE_j c_j s_j(tau) / T.  A pass builds psi with the frames in the ring gathers (qsim_shots_dev.h, FRAMED),
// forms lambda, then per layer in reverse: undoes frame and ring together (one index map and one sign, the same for
// psi and lambda, so a Pauli's overall sign cancels), undoes RZ then RY on every wire of psi and lambda, and takes
// dphi = Im<lambda|Z|psi>, dtheta = Im<lambda|Y|psi> from the pair sums (qsim_gates.h gate_adj).
//
// Determinism: no float atomics.  A workgroup adds its passes' gradients into its own row in pass order, each address
// by one fixed thread.  n >= 10 splits a sample's trajectories over 2, 4 or 8 workgroups as qsim_noise.hip does
// (chunk 0: the shared pass and the rebuilds of its range; chunk c > 0: the rebuilds of its range); they write partial
// rows to `work`, and one small launch sums them in chunk order.  With every threshold zero all T trajectories fall
// into the shared pass with weight T / T = 1 and the other chunks' rows are +0: G does not depend on T, bit for bit.
//
// Layout: psi and lambda both in LDS, 2 x 8 B x 2^n.  n <= 11: at most 34.8 KiB with the trajectory words, inside the
// quarter of a CU's LDS the siblings keep to (kLdsBudget).  n = 12: 64 KiB + at most 2.8 KiB, so TWO workgroups per
// CU, not the siblings' second state in registers (qsim_pshift_dev.h reg_prefix).  Their kept state is only READ, at
// one layout; here lambda goes through every wire's gate in every layer like psi, so held in registers it would
// have to be exchanged through LDS between the layer's qubit groups and again for the ring gather, through the
// buffer psi occupies -- more LDS traffic per layer, to win a third workgroup's occupancy.  That trade has not been
// measured.  The 8-byte accesses, at unit stride in the ring pass and at stride 2^g0 with 2^NB per thread in the
// pair sweeps, are the forward's own pattern (qsim_shots_dev.h apply_layer).
#include "qsim_noise_dev.h"
#include "qsim_pshift_dev.h"

namespace qd {
namespace qnadj {
using namespace qd::qshots;
using namespace qd::qnoise;
using qd::qpshift::group_bits;
using qd::gate_adj;
using qd::ring_fwd;

// LDS carve (bytes): trig (<= 12 float4) | wave partials of the reductions (NW x 2 n floats) | g' (n floats) |
// <Z_j> of the pass (n floats) | psi | lambda | traj words (T)
constexpr int O_RED = 256, O_GW = 640, O_EZ = 704, O_STATE = 768;
template <int N>
constexpr size_t lds_bytes(int T) {
  return O_STATE + 2 * sizeof(cf) * (1 << N) + traj_bytes(T);
}
static_assert(NW * 2 * kMaxQubits * sizeof(float) <= O_GW - O_RED, "the reduction partials fit their slot");
static_assert(lds_bytes<11>(kMaxTraj) <= (size_t)kLdsBudget, "a quarter of a CU's LDS up to n = 11");
static_assert(lds_bytes<12>(kMaxTraj) <= 80 * 1024, "two workgroups per CU at n = 12");

// Qubits per LDS round trip of the reverse sweep.  Two: a thread then holds 4 amplitudes of psi and of lambda.  With
// the forward's three (8 + 8 amplitudes and their gate temporaries) the compiler spilled 680 - 820 bytes per lane at
// n = 9 .. 11 under the four-waves register cap.
#ifndef QD_NADJ_RB
#define QD_NADJ_RB 2
#endif

__device__ __forceinline__ float ro_scale(const uint32_t* thr_ro, int j) {
  return 1.f - (float)(thr_ro[2 * j] + thr_ro[2 * j + 1]) * (1.f / 65536.f);
}
__device__ __forceinline__ float ro_offset(const uint32_t* thr_ro, int j) {
  return ((float)thr_ro[2 * j + 1] - (float)thr_ro[2 * j]) * (1.f / 65536.f);
}
// Ebar from the summed s_j E_j^tau
__device__ __forceinline__ float ebar_of(float sum, const uint32_t* thr_ro, int j, int T) {
  return ro_scale(thr_ro, j) * __fdiv_rn(sum, (float)T) + ro_offset(thr_ro, j);
}

// (waves_per_eu: the workgroups per CU the LDS allows -- two at n = 12 -- except n = 10, 11, where uncapped the
// kernel takes 157 / 179 VGPRs: capped to four waves they spilled 112 / 224 bytes per lane, so three there)
template <int N>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(N >= 12 ? 2 : N >= 10 ? 3 : 4)))
    qsim_nadj_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ gE,
                     float* __restrict__ G, float* __restrict__ Ebar, int* __restrict__ frames_out,
                     float* __restrict__ work, const uint32_t* __restrict__ thr1, const uint32_t* __restrict__ thr2,
                     const uint32_t* __restrict__ thr_ro, int B, int L, int wgroup, int T, unsigned long long seed,
                     unsigned long long ctr0, const unsigned long long* __restrict__ counter) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;
  constexpr int GB = group_bits<N>();
  constexpr int RB = QD_NADJ_RB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  float* red = reinterpret_cast<float*>(smem + O_RED);
  float* gw = reinterpret_cast<float*>(smem + O_GW);
  float* ez = reinterpret_cast<float*>(smem + O_EZ);
  cf* A = reinterpret_cast<cf*>(smem + O_STATE);
  cf* Lm = A + D;
  uint16_t* traj = reinterpret_cast<uint16_t*>(smem + O_STATE + 2 * sizeof(cf) * D);
  const int b = blockIdx.x, chunk = blockIdx.y, nsplit = (int)gridDim.y;
  const int tlo = chunk * (T / nsplit), thi = tlo + T / nsplit;   // the rebuilds this workgroup owns
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int P = 2 * N * L;
  const float* xs = x + (size_t)b * N;
  const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * P : 0);
  const unsigned long long ctr = shot_counter(ctr0, counter);
  const Rng g = {(uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)};
  // this workgroup's row: G's own, or its partial row (P gradients, then n sums for Ebar)
  float* row = work != nullptr ? work + ((size_t)chunk * B + b) * (P + N) : G + (size_t)b * P;

  uint32_t any_gate = 0;   // uniform
#pragma unroll
  for (int q = 0; q < N; ++q) any_gate |= thr1[q] | thr2[q];

  // thread i < 2 n owns row[l 2 n + i] of every layer: it zeroes them here and is the only one to add to them
  if (threadIdx.x < 2 * N)
    for (int l = 0; l < L; ++l) row[l * 2 * N + threadIdx.x] = 0.f;
  float esum = 0.f;   // thread j < n: sum over this workgroup's passes of s_j E_j
  auto store_esum = [&]() {
    if (threadIdx.x < N) {
      if (work != nullptr)
        row[P + threadIdx.x] = esum;
      else if (Ebar != nullptr)
        Ebar[(size_t)b * N + threadIdx.x] = ebar_of(esum, thr_ro, threadIdx.x, T);
    }
  };
  if (chunk > 0 && !any_gate) {   // no frame, so no rebuild: chunk 0 serves every trajectory
    store_esum();
    return;
  }

  // ---- the trajectories' frames: one thread per trajectory (chunk 0 needs every trajectory's word)
  int plain = 0;
  for (int tau = (chunk == 0 ? 0 : tlo) + threadIdx.x; tau < (chunk == 0 ? T : thi); tau += NT) {
    uint16_t word = 0;
    for (int l = 0; l < L; ++l) {
      int fa = 0, fb = 0;
      if (any_gate) {
        const uint32_t f = frame_again<N>(l, (uint32_t)tau, g, thr1, thr2);
        fa = (int)(f & 0xFFFFu);
        fb = (int)(f >> 16);
      }
      if (l < L - 1) {
        if (fa | fb) word |= kRebuild;
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
    plain |= !(word & kRebuild);
  }
  const bool shared_pass = __syncthreads_or(plain) != 0 && chunk == 0;   // (the barrier publishes traj)

  int pass = -1, base = tlo - 64;
  unsigned long long pending = 0;   // the rebuild flags of trajectories base .. base + 63 not yet served (uniform)
  bool first = shared_pass;
  for (;;) {
    if (!first) {   // the next trajectory of the range that rebuilds: 64 flags per LDS read
      while (pending == 0ull) {
        base += 64;
        if (base >= thi) break;
        pending = __ballot(base + lane < thi && (traj[base + lane] & kRebuild));
      }
      if (pending == 0ull) break;
      pass = base + __ffsll((long long)pending) - 1;
      pending &= pending - 1ull;
    }
    first = false;

    // ---- the pass's weights g'_j and the signed trajectory count of wire j (an integer)
    if (threadIdx.x < N) {
      const int j = threadIdx.x;
      int cnt = 0;
      if (pass < 0) {
        for (int tau = 0; tau < T; ++tau) {
          const uint16_t word = traj[tau];
          if (!(word & kRebuild)) cnt += 1 - 2 * ((word >> j) & 1);
        }
      } else {
        cnt = 1 - 2 * ((traj[pass] >> j) & 1);
      }
      gw[j] = gE[(size_t)b * N + j] * ro_scale(thr_ro, j) * __fdiv_rn((float)cnt, (float)T);
      ez[j] = (float)cnt;
    }

    // ---- forward: psi in A, the frames of layers 0 .. L-2 in the ring gathers
    for (int l = 0; l < L; ++l) {
      int fa = 0, fb = 0;
      if (pass >= 0 && l < L - 1) {
        const uint32_t f = frame_again<N>(l, (uint32_t)pass, g, thr1, thr2);
        fa = (int)(f & 0xFFFFu);
        fb = (int)(f >> 16);
      }
      layer_trig(trig, wsmp + 2 * N * l, l == 0 ? xs : nullptr, N);
      __syncthreads();
      if (l == 0)
        product_state<N, true>(A, trig, fa, fb);
      else
        apply_layer<N, GB, 0, true>(A, A, trig, fa, fb);
    }

    // ---- lambda = (sum_j g'_j Z_j) psi; <Z_j> of the pass when Ebar is asked for
    {
      float zs[N];
#pragma unroll
      for (int j = 0; j < N; ++j) zs[j] = 0.f;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int k = threadIdx.x + i * NT;
        if (k < D) {
          const cf a = A[k];
          float o = 0.f;
#pragma unroll
          for (int j = 0; j < N; ++j) o += ((k >> j) & 1) ? -gw[j] : gw[j];
          Lm[k] = cf{o * a.x, o * a.y};
          if (Ebar != nullptr) {
            const float pk = a.x * a.x + a.y * a.y;
#pragma unroll
            for (int j = 0; j < N; ++j) zs[j] += ((k >> j) & 1) ? -pk : pk;
          }
        }
      }
      if (Ebar != nullptr) {   // uniform
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float s = wave_sum(zs[j]);
          if (lane == 0) red[wv * N + j] = s;
        }
        __syncthreads();
        if (threadIdx.x < N) {
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < NW; ++k) s += red[k * N + threadIdx.x];
          esum += ez[threadIdx.x] * s;
        }
      }
      __syncthreads();   // lambda is complete; red and gw may be rewritten
    }

    // ---- reverse sweep
    for (int l = L - 1; l >= 0; --l) {
      int fa = 0, fb = 0;
      if (pass >= 0 && l < L - 1) {
        const uint32_t f = frame_again<N>(l, (uint32_t)pass, g, thr1, thr2);
        fa = (int)(f & 0xFFFFu);
        fb = (int)(f >> 16);
      }
      layer_trig(trig, wsmp + 2 * N * l, l == 0 ? xs : nullptr, N);
      // undo frame and ring: the forward put sign(fb, js) A_gates[k] at j = js ^ fa, js = f(k)
      {
        cf p[PER], m[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int k = threadIdx.x + i * NT;
          if (k < D) {
            const int js = ring_fwd<N>(k);
            p[i] = frame_sign(A[js ^ fa], fb, js);
            m[i] = frame_sign(Lm[js ^ fa], fb, js);
          }
        }
        __syncthreads();   // (also publishes trig)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int k = threadIdx.x + i * NT;
          if (k < D) {
            A[k] = p[i];
            Lm[k] = m[i];
          }
        }
        __syncthreads();
      }
      // undo the layer's gates, RB qubits per LDS round trip (they act on different wires, so the groups commute)
      float dth[N], dph[N];
#pragma unroll
      for (int q = 0; q < N; ++q) dth[q] = dph[q] = 0.f;
      static_for<0, (N + RB - 1) / RB>([&](auto gc) {
        constexpr int g0 = RB * decltype(gc)::value;
        constexpr int NB = (N - g0) < RB ? (N - g0) : RB;
        for (int t = threadIdx.x; t < (D >> NB); t += NT) {
          const int bs = ((t >> g0) << (g0 + NB)) | (t & ((1 << g0) - 1));
          cf p[1 << NB], m[1 << NB];
#pragma unroll
          for (int j = 0; j < (1 << NB); ++j) {
            p[j] = A[bs | (j << g0)];
            m[j] = Lm[bs | (j << g0)];
          }
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            const float4 tg = trig[g0 + q];
#pragma unroll
            for (int j = 0; j < (1 << NB); ++j)
              if (!((j >> q) & 1)) gate_adj(p[j], p[j | (1 << q)], m[j], m[j | (1 << q)], tg, dth[g0 + q], dph[g0 + q]);
          }
          if (l > 0) {   // (layer 0 ends in |0..0>: nothing reads it)
#pragma unroll
            for (int j = 0; j < (1 << NB); ++j) {
              A[bs | (j << g0)] = p[j];
              Lm[bs | (j << g0)] = m[j];
            }
          }
        }
        __syncthreads();
      });
      // the layer's 2 n sums over the block, in a fixed order, into the row
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const float st = wave_sum(dth[q]), sp = wave_sum(dph[q]);
        if (lane == 0) {
          red[wv * 2 * N + 2 * q] = st;
          red[wv * 2 * N + 2 * q + 1] = sp;
        }
      }
      __syncthreads();
      if (threadIdx.x < 2 * N) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) s += red[k * 2 * N + threadIdx.x];
        row[l * 2 * N + threadIdx.x] += s;
      }
      __syncthreads();   // red and trig may be rewritten
    }
  }
  store_esum();
}

// Split grid: the chunks' partial rows, summed in chunk order -> G and Ebar.
__global__ void nadj_finalize_kernel(const float* __restrict__ work, float* __restrict__ G, float* __restrict__ Ebar,
                                     const uint32_t* __restrict__ thr_ro, int B, int P, int n, int nsplit, int T) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int R = P + n;
  if (i >= (long long)B * R) return;
  const int b = (int)(i / R), c = (int)(i % R);
  float s = work[i];
  for (int k = 1; k < nsplit; ++k) s += work[(size_t)k * B * R + i];
  if (c < P)
    G[(size_t)b * P + c] = s;
  else if (Ebar != nullptr)
    Ebar[(size_t)b * n + (c - P)] = ebar_of(s, thr_ro, c - P, T);
}

template <int N>
static int launch(const float* x, const float* w, const float* gE, float* G, float* Ebar, int* frames_out, float* work,
                  const uint32_t* thr1, const uint32_t* thr2, const uint32_t* thr_ro, int B, int L, int wgroup, int T,
                  int nsplit, unsigned long long seed, unsigned long long ctr0, const unsigned long long* counter,
                  hipStream_t st) {
  const size_t sm = lds_bytes<N>(T);
  if (hipError_t e = allow_lds(qsim_nadj_kernel<N>, sm)) return (int)e;
  hipLaunchKernelGGL((qsim_nadj_kernel<N>), dim3(B, nsplit), dim3(NT), sm, st, x, w, gE, G, Ebar, frames_out,
                     nsplit > 1 ? work : nullptr, thr1, thr2, thr_ro, B, L, wgroup, T, seed, ctr0, counter);
  if (hipError_t e = hipGetLastError()) return (int)e;
  if (nsplit > 1) {
    const long long total = (long long)B * (2 * N * L + N);
    hipLaunchKernelGGL(nadj_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, work, G, Ebar,
                       thr_ro, B, 2 * N * L, N, nsplit, T);
  }
  return (int)hipGetLastError();
}

}  // namespace qnadj
}  // namespace qd

// The chunks per sample qd_qsim_noisy_adjoint launches for T trajectories of n qubits (0: T out of range).  More
// than one needs a `work` buffer of chunks x B x (2 n L + n) floats.
QD_API int qd_qsim_nadj_split(int T, int n) {
  return T >= 1 && T <= qd::qnoise::kMaxTraj ? qd::qnoise::choose_split(T, n) : 0;
}

// G (B, 2 n L) fp32; Ebar (nullable; B, n) fp32; frames_out (nullable; B, T, L, 2) int32: every layer's (a, b).
// x (B, n), w (L, n, 2) or grouped (wgroup samples per group), gE (B, n); thr1 / thr2 (n) uint32 gate thresholds,
// thr_ro (n, 2) uint32 readout thresholds (<= 65535).  work: qd_qsim_nadj_split(T, n) x B x (2 n L + n) floats when
// that split is above 1 (else unused, nullable).  counter (nullable): device uint64 added to ctr0; read only.
QD_API int qd_qsim_noisy_adjoint(const float* x, const float* w, const float* gE, float* G, float* Ebar,
                                 int* frames_out, float* work, const void* thr1, const void* thr2, const void* thr_ro,
                                 int B, int n, int L, int wgroup, int T, unsigned long long seed,
                                 unsigned long long ctr0, const void* counter, void* stream) {
  using namespace qd::qnoise;
  if (!noisy_args_ok(n, B, L, wgroup, T, thr1, thr2, thr_ro)) return (int)hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || gE == nullptr || G == nullptr) return (int)hipErrorInvalidValue;
  const int nsplit = qd::qnoise::choose_split(T, n);
  if (nsplit > 1 && work == nullptr) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) {
    return qd::qnadj::launch<N>(x, w, gE, G, Ebar, frames_out, work, (const uint32_t*)thr1, (const uint32_t*)thr2,
                                (const uint32_t*)thr_ro, B, L, wgroup, T, nsplit, seed, ctr0,
                                (const unsigned long long*)counter, (hipStream_t)stream);
  });
}
