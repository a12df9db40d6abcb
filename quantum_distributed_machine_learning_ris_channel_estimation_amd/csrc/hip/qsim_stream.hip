// Streamed VQC simulator for HBM-resident states (n = 13 .. 16 qubits, L >= 2 layers).
//
// Same circuit and adjoint method as csrc/hip/qsim.hip / qsim_big.hip (reference E:125-142: RY
// angle embedding, L x [RY, RZ on every wire, CNOT ring], <Z_i>).  qsim_big.hip gives each sample ONE
// 256-thread workgroup that walks its 2^n-amplitude state (512 KiB at n = 16) pass after pass: a few
// KiB in flight per CU, measured 1.2-1.8 TB/s on the forward and backward of the 16-qubit flagship
// config (profiles/r2_11_q16_*).  Here every pass is its own launch over ALL samples at once, one
// workgroup per (sample, 4096-amplitude brick) -- 36,864 workgroups at n = 16, B = 2304 -- so each
// pass streams the whole batch's state at HBM rate:
//
//   pass A   qubits {0..7} u {12..n-1}: the brick is 2^(n-12) runs of 256 contiguous amplitudes
//            (bits 8..11 fixed = brick index).  A thread handles the bits it holds from its coalesced
//            16-byte loads (bit 0 and the bits above its load stride) in registers; the other bits
//            go through a padded LDS image in two groups of up to four.
//   pass B   qubits {8..11} + the CNOT ring: the brick is the contiguous tile of bits 0..11 (one
//            thread owns the 16 amplitudes that differ in bits 8..11: the 4 rotations stay in
//            registers).  The ring f is GF(2)-linear (bit j of f(k) = parity of bits 0..j, bit 0 =
//            parity of bits 1..n-1), so f maps a tile onto exactly TWO runs of 2048 contiguous
//            amplitudes (selected by bit 11 of the image): the permutation is an LDS scatter, and
//            every global load and store of both passes is coalesced.
//
// Forward (L layers): pass A of layer 1 GENERATES its input (the ring image of the layer-0 product
// state) instead of loading it, then B, A, B, ...; every pass A's output S_l is KEPT (the backward's
// psi, round 3: HBM has room -- 1.2 GB per state at n = 16, B = 2304), the passes B write a scratch
// state, and the last pass B stores nothing: it only reduces the per-tile <Z_q> partials.  Both passes
// apply RY alone bit by bit and the pass's RZ gates as ONE phase per amplitude afterwards (RZ of a qubit
// commutes with every other qubit's RY): the 16-qubit forward 1.61 instead of 1.72 ms (profiles/r6_31_*).
// Backward: per layer in reverse, pass B (lambda gathered at the ring image, psi = S_l with the layer's
// rotations 8..11 re-applied in registers; d(theta), d(phi) partials of qubits 8..11, lambda undone) and pass A
// (psi = S_l, the rest); only lambda is written -- psi is never un-applied, in registers, LDS or memory:
// every d(phi_b) is Im<lambda| Z_b |psi> and every d(theta_b) a pair sum <lambda| G_b |psi> of the states as
// loaded (the pass's RZ phases undone, one phase per amplitude), because Z_b and G_b commute with the
// pass's gates on the other qubits and with their own.  Layer 0's
// psi is the product state, generated in-kernel; once its qubits 8..11 are undone it is zero outside the
// brick whose bits 8..11 are 0, so layer 0's pass B stores only that part of lambda and its pass A reads
// only that brick.  lambda = (sum_q g_q Z_q) psi_final is formed in registers by the first pass B (psi_final
// at the ring image of a tile = that tile's rotated psi).  Gradient partials go to a slab of 16 rows per
// sample (every column written once per row): the caller's slab reduction sums them; dx = the layer-0
// theta columns, reduced per sample here.
//
// State traffic at n = 16, L = 3 (1.2 GB per state): forward 6 state passes, backward ~12 (round 2: 7 and
// 21, with psi un-applied and re-stored in every backward pass).
//
// The pass forms that round 6 measured and replaced (bit-by-bit LDS sweeps, the two-tile reverse passes,
// gate-by-gate RZ, 2 / 4 bricks per workgroup, the chunked backward) are in the history, not here: README.md
// "Round 6" and "Measured in round 6 and not adopted" give their numbers and the last commit that builds them.
#include "qsim_gates.h"
#include "qsim_shots_dev.h"   // prob_of, quantise: the finite-shot contract's fp32 probability and its 2^30 word

namespace qd {
namespace qstream {
using qd::cf;
using qd::cmul;
using qd::gate_fwd;
using qd::ins_bits;
using qd::ring_fwd_scan;   // (the ring in closed form: the streamed passes were tuned with it)
using qd::ring_inv_scan;

constexpr int NT = 256;
constexpr int NWV = NT / 64;
constexpr int ROWS = 16;   // slab rows (workgroups of pass A) per sample


template <int N>
struct SG {
  static constexpr int HB = N - 12;        // bits above the 4096-amplitude tile
  static constexpr int D = 1 << N;
  static constexpr int AB = 8 + HB;        // pass-A brick bits (qubits 0..7 and 12..N-1)
  static constexpr int AS = 1 << AB;       // pass-A brick size
  static constexpr int NTILE = 1 << HB;    // pass-B tiles per sample
  // threads of the adjoint pass A: one 3-qubit set (8 amplitudes) each, at most 256
  static constexpr int NTA = AS / 8 < 256 ? AS / 8 : 256;
  static_assert(N >= 13 && N <= 16, "streamed simulator: 13..16 qubits");
};

// pass-A brick element e -> state index (brick = bits 8..11)
__device__ __forceinline__ int brick_k(int e, int br) { return (e & 255) | (br << 8) | ((e >> 8) << 12); }
// pass-A brick bit -> qubit
__device__ __forceinline__ constexpr int brick_q(int b) { return b < 8 ? b : b + 4; }

// Layer-0 product state (embedding + layer-0 rotations on |0..0>, BEFORE its ring) as two tables: amplitude
// of basis state k = PL[k & 255] * PH[k >> 8] (qubits 0..7 / 8..N-1).  Qubits in `zero` (a mask) are taken
// back to |0> (their gates already undone by the adjoint).  trig0: layer-0 (cos, sin) per qubit.  NTH threads
// (any count: the 256 entries are strided over them).
template <int N, int NTH>
__device__ __forceinline__ void product_tables(const float4* trig0, cf* PL, cf* PH, int zero) {
  for (int i = threadIdx.x; i < 256; i += NTH) {
    cf a = {1.f, 0.f}, h = {1.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 t = trig0[q];
      const bool one = (i >> q) & 1;
      const cf f = ((zero >> q) & 1) ? cf{one ? 0.f : 1.f, 0.f}
                                     : (one ? cf{t.y * t.z, t.y * t.w} : cf{t.x * t.z, -t.x * t.w});
      a = cmul(a, f);
    }
#pragma unroll
    for (int q = 8; q < N; ++q) {
      const float4 t = trig0[q];
      const bool one = (i >> (q - 8)) & 1;
      const cf f = ((zero >> q) & 1) ? cf{one ? 0.f : 1.f, 0.f}
                                     : (one ? cf{t.y * t.z, t.y * t.w} : cf{t.x * t.z, -t.x * t.w});
      h = cmul(h, f);
    }
    PL[i] = a;
    if (i < (1 << (N - 8))) PH[i] = h;
  }
}

// RY(theta) alone on the pair (the forward's RZ phases are applied afterwards, one per amplitude)
__device__ __forceinline__ void gate_ry(cf& a0, cf& a1, float4 t) {
  const cf t0 = {t.x * a0.x - t.y * a1.x, t.x * a0.y - t.y * a1.y};
  const cf t1 = {t.y * a0.x + t.x * a1.x, t.y * a0.y + t.x * a1.y};
  a0 = t0;
  a1 = t1;
}

// (cos, sin) of theta/2 and phi/2 of layer l for every qubit of sample s (theta + x at layer 0)
template <int N>
__device__ __forceinline__ void load_trig(float4* trig, const float* x, const float* w, int s, int L, int l,
                                          int wgroup) {
  if (threadIdx.x < N) {
    const int q = threadIdx.x;
    const float* wl = w + (wgroup > 0 ? (size_t)(s / wgroup) * 2 * N * L : 0) + 2 * N * l;
    float sn, c, sp, cp;
    __sincosf(0.5f * (wl[2 * q] + (l == 0 ? x[(size_t)s * N + q] : 0.f)), &sn, &c);
    __sincosf(0.5f * wl[2 * q + 1], &sp, &cp);
    trig[q] = make_float4(c, sn, cp, sp);
  }
}

// dst[i] = sum over the workgroup of v[i] (thread 0..NV-1 hold the results); red: NWV * NV floats
template <int NV, int NTH = NT>
__device__ __forceinline__ void block_sum_vec(const float (&v)[NV], float* red, float* out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum(v[i]);
    if (lane == 0) red[w * NV + i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NTH / 64; ++k) s += red[k * NV + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// LDS image of the layer-0 reverse pass A: one pad amplitude per 8 (element e at e + e / 8).  Unpadded, a wave's
// 8-byte accesses 64 bytes apart hit 4 bank pairs: 8-way conflicts.  The pad was chosen for sweeps in which a thread
// owned 8 contiguous or 8-strided amplitudes, and stays: the images' size is part of the launch (Smem::A_BWD).
__device__ __forceinline__ int padx(int e) { return e + (e >> 3); }
constexpr int ilog2c(int v) { return v <= 1 ? 0 : 1 + ilog2c(v >> 1); }

// Every d(theta) of the layer-0 reverse pass A (bits 0 .. NBITS-1 of the padx images of psi, tp, and lambda, tq;
// brick_q qubit map; the pass's RZ phases were undone -- and every d(phi) taken -- when the brick was loaded).  Every
// d(theta_b) is a pair sum <lambda| G_b |psi> with G_b acting on qubit b alone, and G_b commutes with every RY of the
// layer (the other qubits' and its own: same axis), so all of them come from the brick as loaded, in one read-only pass
// over 4-bit groups; nothing is undone or written back (layer 0's lambda is not stored: nothing reads it).  Each
// group's partials are reduced over the wave and added to this wave's slot of wacc (2 NBITS floats per wave, lane 0
// of a wave its slot's only writer).  Ends with a barrier: every wave's slot is final.
template <int TOT, int NBITS, int NTH>
__device__ __forceinline__ void lds_dtheta(cf* tp, cf* tq, float* wacc) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int NG4 = (NBITS + 3) / 4;
  static_for<0, NG4>([&](auto gc) {
    constexpr int r0 = 4 * decltype(gc)::value;
    constexpr int NB = (NBITS - r0) < 4 ? (NBITS - r0) : 4;
    constexpr int ACT = (1 << TOT) >> NB;
    float dth[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) dth[b] = 0.f;
#pragma unroll 1
    for (int t = threadIdx.x; t < ACT; t += NTH) {
      const int base = ins_bits<r0, NB>(t);
      cf p[1 << NB], m[1 << NB];
#pragma unroll
      for (int j = 0; j < (1 << NB); ++j) {
        p[j] = tp[padx(base | (j << r0))];
        m[j] = tq[padx(base | (j << r0))];
      }
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < (1 << NB); ++j)
          if (!((j >> b) & 1)) {
            const cf p0 = p[j], p1 = p[j | (1 << b)], l0 = m[j], l1 = m[j | (1 << b)];
            dth[b] += -(l0.x * p1.x + l0.y * p1.y) + (l1.x * p0.x + l1.y * p0.y);
          }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float s1 = wave_sum(dth[b]);
      if (lane == 0) wacc[wv * 2 * NBITS + 2 * (r0 + b)] += s1;
    }
  });
  __syncthreads();
}

// LDS image of the other passes A (forward, and reverse at layers l > 0): two pad amplitudes per 32, so a half-wave of
// the group on bits 1..4 -- lanes 32 amplitudes apart, and bit 0 -- hits 32 distinct 8-byte slots; with one per 32,
// pairs of lanes shared a slot: 22 % of the pass's LDS cycles were bank conflicts (profiles/r6_35_qstream_pmc_b.md;
// 16-qubit backward 3.42 instead of 3.51 ms, profiles/r6_36_*).  The index math and the image sizes (Smem) use PADQ.
constexpr int PADQ = 2;
__device__ __forceinline__ int padq(int e) { return e + PADQ * (e >> 5); }
// a 16-byte aligned pair of amplitudes in an LDS image (even padq index): one ds_read_b128 / ds_write_b128 per lane
// instead of the ds_read2_b64 / ds_write2_b64 the compiler forms from two 8-byte accesses (whose banks wrap every
// 32 dwords: 4x the LDS cycles of b128 for the same 16 bytes)
__device__ __forceinline__ float4* lds16(cf* p) { return reinterpret_cast<float4*>(__builtin_assume_aligned(p, 16)); }

// RY^dagger on bits [LO, LO + NB) of lambda's padq image tq (the reverse pass A at l > 0: psi is never undone and
// every d(theta) was taken before, so lambda alone is read), one sweep: 8 vector operations per pair and bit.  OUT:
// 1 = lambda back to LDS, 2 = lambda straight to its state in HBM (gdst, brick br: for a fixed register index the lanes
// hold runs of 32 consecutive amplitudes, 256-byte pieces of the state).  Ends with a barrier.
template <int TOT, int LO, int NB, int NTH, int OUT>
__device__ __forceinline__ void lds_group_lam(cf* tq, const float4* trig, cf* gdst = nullptr, int br = 0) {
  static_assert(OUT == 1 || OUT == 2, "lambda to LDS or to HBM");
  constexpr int ACT = (1 << TOT) >> NB;
  // the group's amplitudes sit at padq(base) + j STR: base has the group's bits clear, so with the group below bit 5
  // or from bit 5 up no carry crosses the pad (one address register, the rest immediate offsets)
  static_assert(LO + NB <= 5 || LO >= 5, "a group either below or from bit 5");
  constexpr int STR = (1 << LO) + PADQ * ((1 << LO) >> 5);
#pragma unroll 1
  for (int t = threadIdx.x; t < ACT; t += NTH) {
    const int eb = ins_bits<LO, NB>(t), pb = padq(eb);
    cf m[1 << NB];
#pragma unroll
    for (int j = 0; j < (1 << NB); ++j) m[j] = tq[pb + j * STR];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 tg = trig[brick_q(LO + b)];
#pragma unroll
      for (int j = 0; j < (1 << NB); ++j)
        if (!((j >> b) & 1)) {
          const cf m0 = m[j], m1 = m[j | (1 << b)];
          m[j] = {tg.x * m0.x + tg.y * m1.x, tg.x * m0.y + tg.y * m1.y};
          m[j | (1 << b)] = {tg.x * m1.x - tg.y * m0.x, tg.x * m1.y - tg.y * m0.y};
        }
    }
#pragma unroll
    for (int j = 0; j < (1 << NB); ++j) {
      if constexpr (OUT == 2)
        *reinterpret_cast<float2*>(gdst + brick_k(eb | (j << LO), br)) = make_float2(m[j].x, m[j].y);
      else
        tq[pb + j * STR] = m[j];
    }
  }
  __syncthreads();
}

// The forward counterpart (pass A): RY on bits [LO, LO + NB) of the LDS brick, one sweep; TOG: the result straight to
// the state in HBM (gdst, brick br) instead of back to LDS, every amplitude multiplied on the way by the pass's whole
// RZ diagonal ZL[e & 255] ZH[e >> 8] (RZ of a qubit commutes with every other qubit's RY, so the phases may wait for
// the last RY).
template <int TOT, int LO, int NB, int NTH, bool TOG>
__device__ __forceinline__ void lds_group_fwd(cf* tp, const float4* trig, cf* gdst = nullptr, int br = 0,
                                              const cf* ZL = nullptr, const cf* ZH = nullptr) {
  constexpr int ACT = (1 << TOT) >> NB;
  static_assert(LO + NB <= 5 || LO >= 5, "a group either below or from bit 5");
  constexpr int STR = (1 << LO) + PADQ * ((1 << LO) >> 5);
#pragma unroll 1
  for (int t = threadIdx.x; t < ACT; t += NTH) {
    const int eb = ins_bits<LO, NB>(t), pb = padq(eb);
    cf p[1 << NB];
#pragma unroll
    for (int j = 0; j < (1 << NB); ++j) p[j] = tp[pb + j * STR];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 tg = trig[brick_q(LO + b)];
#pragma unroll
      for (int j = 0; j < (1 << NB); ++j)
        if (!((j >> b) & 1)) gate_ry(p[j], p[j | (1 << b)], tg);
    }
#pragma unroll
    for (int j = 0; j < (1 << NB); ++j) {
      if constexpr (TOG) {
        const int e = eb | (j << LO);
        const cf v = cmul(p[j], cmul(ZL[e & 255], ZH[e >> 8]));
        *reinterpret_cast<float2*>(gdst + brick_k(e, br)) = make_float2(v.x, v.y);
      } else {
        tp[pb + j * STR] = p[j];
      }
    }
  }
  if constexpr (!TOG) __syncthreads();
}

// ------------------------------------------------------------------------------------------ forward
// pass A of layer l (GEN: layer 1, its input generated: the ring image of the layer-0 product state).  The bits a
// thread holds from its coalesced loads (bit 0 and bits RLO.., 2 NT apart) in registers, the rest in two LDS groups,
// the second storing straight to HBM: 2 LDS sweeps and their barriers (layer 1's generating pass at n = 16 436 instead
// of 514 us in four 3-bit sweeps + a store loop, profiles/r6_25_*).
template <int N, bool GEN>
__global__ void __launch_bounds__(NT, 2) pass_a_fwd(const float* __restrict__ x, const float* __restrict__ w, int L,
                                                 int l, int wgroup, const cf* __restrict__ in, cf* __restrict__ out) {
  using C = SG<N>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);          // 16
  float4* trig0 = trig + 16;                                 // 16 (GEN)
  cf* tp = reinterpret_cast<cf*>(smem + 512);
  const int br = blockIdx.x, s = blockIdx.y;
  constexpr int NPAIR = C::AS / (2 * NT), RLO = ilog2c(2 * NT), NRB = 1 + ilog2c(NPAIR);
  static_assert(C::AS % (2 * NT) == 0, "whole float4 rounds");
  // (not GEN) the brick's loads issued first: in flight across the angle loads and the tables (behind them they
  // were a second round trip per workgroup)
  [[maybe_unused]] float4 v0[NPAIR];
  if constexpr (!GEN) {
    const cf* si = in + (size_t)s * C::D;
#pragma unroll
    for (int i = 0; i < NPAIR; ++i)
      v0[i] = *reinterpret_cast<const float4*>(si + brick_k(2 * threadIdx.x + 2 * NT * i, br));
  }
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  if constexpr (GEN) load_trig<N>(trig0, x, w, s, L, 0, wgroup);
  __syncthreads();
  cf* st = out + (size_t)s * C::D;
  // the pass's RZ diagonal: ZL over brick bits 0..7, ZH over 8.. (qubit q's factor cos(phi/2) -+ i sin(phi/2),
  // - for bit 0), right past the padded image (the GEN tables after them: without them the pass holds 37.5 KB of
  // LDS, four workgroups per CU); read by the last group after two barriers
  cf* ZLf = tp + C::AS + PADQ * (C::AS / 32);
  cf* ZHf = ZLf + 256;
  {
    const int i = threadIdx.x;
    cf a = {1.f, 0.f};
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const float4 tq4 = trig[b];
      a = cmul(a, cf{tq4.z, ((i >> b) & 1) ? tq4.w : -tq4.w});
    }
    ZLf[i] = a;
    if (i < (1 << (C::AB - 8))) {
      cf h = {1.f, 0.f};
#pragma unroll
      for (int b = 8; b < C::AB; ++b) {
        const float4 tq4 = trig[brick_q(b)];
        h = cmul(h, cf{tq4.z, ((i >> (b - 8)) & 1) ? tq4.w : -tq4.w});
      }
      ZHf[i] = h;
    }
  }
  cf p[2 * NPAIR];
  if constexpr (GEN) {   // the ring image of the layer-0 product state, generated in registers
    cf* PL = tp + C::AS + PADQ * (C::AS / 32) + 256 + 16;   // (past the padded image and the RZ tables)
    cf* PH = PL + 256;
    product_tables<N, NT>(trig0, PL, PH, 0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2 * NPAIR; ++j) {
      const int k = ring_inv_scan<N>(brick_k(2 * threadIdx.x + 2 * NT * (j >> 1) + (j & 1), br));
      p[j] = cmul(PL[k & 255], PH[k >> 8]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      p[2 * i] = cf{v0[i].x, v0[i].y};
      p[2 * i + 1] = cf{v0[i].z, v0[i].w};
    }
  }
#pragma unroll
  for (int b = 0; b < NRB; ++b) {
    const float4 tg = trig[brick_q(b == 0 ? 0 : RLO + b - 1)];
#pragma unroll
    for (int j = 0; j < 2 * NPAIR; ++j)
      if (!((j >> b) & 1)) gate_ry(p[j], p[j | (1 << b)], tg);
  }
  const int pb = padq(2 * threadIdx.x);
#pragma unroll
  for (int i = 0; i < NPAIR; ++i)
    *lds16(tp + pb + i * (2 * NT + PADQ * ((2 * NT) / 32))) = make_float4(p[2 * i].x, p[2 * i].y, p[2 * i + 1].x,
                                                                           p[2 * i + 1].y);
  __syncthreads();
  constexpr int NB1 = RLO - 1 < 4 ? RLO - 1 : 4;
  static_assert(RLO > 1 + NB1, "two LDS groups");
  constexpr int NB2 = (C::AB < RLO ? C::AB : RLO) - 1 - NB1;   // (n = 13: the brick ends at bit 8)
  lds_group_fwd<C::AB, 1, NB1, NT, false>(tp, trig);
  lds_group_fwd<C::AB, 1 + NB1, NB2, NT, true>(tp, trig, st, br, ZLf, ZHf);
}

// pass B of layer l: qubits 8..11 in registers (RY per bit, then their four RZ as one phase per amplitude), the ring
// as an LDS scatter, two coalesced output runs.
// LAST: only the per-tile <Z_q> partials epart[(s * NTILE + t) * N + q] (no state store, no LDS scatter).
template <int N, bool LAST>
__global__ void __launch_bounds__(NT, 2) pass_b_fwd(const float* __restrict__ x, const float* __restrict__ w, int L,
                                                 int l, int wgroup, const cf* __restrict__ in, cf* __restrict__ out,
                                                 float* __restrict__ epart) {
  using C = SG<N>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);
  float* red = reinterpret_cast<float*>(smem + 256);          // NWV * N floats
  cf* tp = reinterpret_cast<cf*>(smem + 512);
  const int t = blockIdx.x, s = blockIdx.y, c = threadIdx.x;
  // the tile's loads first: in flight across the angle loads (behind them, a second round trip for wave 0 that the
  // barrier below made every wave wait out)
  const cf* src = in + (size_t)s * C::D + ((size_t)t << 12);
  cf a[16];
#pragma unroll
  for (int h = 0; h < 16; ++h) a[h] = src[(h << 8) | c];
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  // (not LAST) the four RZ of qubits 8..11 as one phase per amplitude: ZT[h] built by threads 0..15 from the
  // weights directly, so the one barrier below covers it too.  LAST: the phases do not change |amplitude|^2 -- none.
  [[maybe_unused]] cf* ZT = reinterpret_cast<cf*>(smem + 512 - 16 * sizeof(cf));
  if constexpr (!LAST) {
    if (threadIdx.x < 16) {
      const float* wl = w + (wgroup > 0 ? (size_t)(s / wgroup) * 2 * N * L : 0) + 2 * N * l;
      cf z = {1.f, 0.f};
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float sp, cp;
        __sincosf(0.5f * wl[2 * (8 + b) + 1], &sp, &cp);
        z = cmul(z, cf{cp, ((threadIdx.x >> b) & 1) ? sp : -sp});
      }
      ZT[threadIdx.x] = z;
    }
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float4 tg = trig[8 + b];
#pragma unroll
    for (int h = 0; h < 16; ++h)
      if (!((h >> b) & 1)) gate_ry(a[h], a[h | (1 << b)], tg);
  }
  if constexpr (LAST) {
    // <Z_q> straight from the registers: amplitude k = (t << 12) | (h << 8) | c lands at j = ring(k), and bit q of j
    // is the parity of k's bits 0..q (bit 0: of bits 1..N-1) -- for q <= 7 this thread's constant, for q = 8..11 that
    // constant times a sign pattern over h, above that also the tile's -- so 5 signed sums of |a_h|^2 give all N
    // partials (no ring scatter through LDS, no barrier, no 16-way sign loop per amplitude)
    float S = 0.f, Sh[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      const float pw = a[h].x * a[h].x + a[h].y * a[h].y;
      S += pw;
#pragma unroll
      for (int m = 0; m < 4; ++m) Sh[m] += (__builtin_popcount(h & ((2 << m) - 1)) & 1) ? -pw : pw;
    }
    const int pc = __popc(c & 255) & 1;   // parity of k's bits 0..7
    float part[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (q == 0) {
        const int par = (__popc(c & 254) + __popc(t)) & 1;   // bits 1..7 and the tile's; h's parity in Sh[3]
        part[q] = par ? -Sh[3] : Sh[3];
      } else if (q < 8) {
        part[q] = (__popc(c & ((2 << q) - 1)) & 1) ? -S : S;
      } else if (q < 12) {
        part[q] = pc ? -Sh[q - 8] : Sh[q - 8];
      } else {
        const int par = (pc + __popc(t & ((2 << (q - 12)) - 1))) & 1;
        part[q] = par ? -Sh[3] : Sh[3];
      }
    }
    float o[N];
    block_sum_vec<N>(part, red, o);
    if (threadIdx.x < N) epart[((size_t)s * C::NTILE + t) * N + threadIdx.x] = o[threadIdx.x];
    return;
  }
#pragma unroll
  for (int h = 0; h < 16; ++h) a[h] = cmul(a[h], ZT[h]);
#pragma unroll
  for (int h = 0; h < 16; ++h) tp[ring_fwd_scan<N>((t << 12) | (h << 8) | c) & 4095] = a[h];
  __syncthreads();
  const int A0 = ring_fwd_scan<N>(t << 12) >> 12, A1 = ring_fwd_scan<N>((t << 12) | 2048) >> 12;
  cf* dst = out + (size_t)s * C::D;
  // (a dead array, left from the <Z_q> reduction this loop once carried: the compiler drops it, but without it the
  // same instructions come out in another order, and the pruning of this file's A/B variants kept every kernel byte
  // for byte.  Taking it out is a change to measure.)
  float part[N];
#pragma unroll
  for (int q = 0; q < N; ++q) part[q] = 0.f;
  for (int i = 2 * threadIdx.x; i < 4096; i += 2 * NT) {
    const int j = i | ((i & 2048 ? A1 : A0) << 12);
    const float4 v = *reinterpret_cast<const float4*>(tp + i);
    *reinterpret_cast<float4*>(dst + j) = v;
  }
}

// The probabilities pass (finite shots at n = 13..16, csrc/hip/qsim_stream_shots.hip): the forward's last pass B with
// the ring scatter of the non-last pass and |amplitude|^2 (qshots::prob_of: explicit roundings) stored instead of a
// state -- probs[s * D + j] fp32 in natural order, the tile's two coalesced runs of 2048 with 16-byte stores.  RY on
// qubits 8..11 only: the layer's RZ phases leave |a|^2 alone (as pass_b_fwd's LAST branch).  RT: runtot[s, j >> 11] =
// the uint32 sum of qshots::quantise(p) over each of the two runs; the ring maps the sample's tiles one-to-one onto
// its 2^(N-11) runs, so every run total is written once, by one workgroup.
template <int N, bool RT>
__global__ void __launch_bounds__(NT, 2) pass_b_probs(const float* __restrict__ x, const float* __restrict__ w, int L,
                                                   int l, int wgroup, const cf* __restrict__ in,
                                                   float* __restrict__ probs, uint32_t* __restrict__ runtot) {
  using C = SG<N>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);
  uint32_t* red = reinterpret_cast<uint32_t*>(smem + 256);    // NWV * 2 words
  cf* tp = reinterpret_cast<cf*>(smem + 512);
  const int t = blockIdx.x, s = blockIdx.y, c = threadIdx.x;
  const cf* src = in + (size_t)s * C::D + ((size_t)t << 12);
  cf a[16];
#pragma unroll
  for (int h = 0; h < 16; ++h) a[h] = src[(h << 8) | c];
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float4 tg = trig[8 + b];
#pragma unroll
    for (int h = 0; h < 16; ++h)
      if (!((h >> b) & 1)) gate_ry(a[h], a[h | (1 << b)], tg);
  }
#pragma unroll
  for (int h = 0; h < 16; ++h) tp[ring_fwd_scan<N>((t << 12) | (h << 8) | c) & 4095] = a[h];
  __syncthreads();
  const int A0 = ring_fwd_scan<N>(t << 12) >> 12, A1 = ring_fwd_scan<N>((t << 12) | 2048) >> 12;
  float* dst = probs + (size_t)s * C::D;
  uint32_t rt[2] = {0u, 0u};
#pragma unroll
  for (int u = 0; u < 4; ++u) {   // u = 0, 1: the run below bit 11 of the image; 2, 3: the run above
    const int i = 4 * c + 4 * NT * u;
    const float4 v0 = *lds16(tp + i), v1 = *lds16(tp + i + 2);
    const float4 p = make_float4(qshots::prob_of(qshots::cf{v0.x, v0.y}), qshots::prob_of(qshots::cf{v0.z, v0.w}),
                                 qshots::prob_of(qshots::cf{v1.x, v1.y}), qshots::prob_of(qshots::cf{v1.z, v1.w}));
    *reinterpret_cast<float4*>(dst + (i | ((u >> 1 ? A1 : A0) << 12))) = p;
    if constexpr (RT)
      rt[u >> 1] += qshots::quantise(p.x) + qshots::quantise(p.y) + qshots::quantise(p.z) + qshots::quantise(p.w);
  }
  if constexpr (RT) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) rt[r] += __shfl_xor(rt[r], m);
      if (lane == 0) red[wv * 2 + r] = rt[r];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < NWV; ++k) o += red[k * 2 + threadIdx.x];
      runtot[(size_t)s * (2 * C::NTILE) + 2 * (threadIdx.x ? A1 : A0) + threadIdx.x] = o;
    }
  }
}

template <int N>
__global__ void __launch_bounds__(256) reduce_e(const float* __restrict__ epart, float* __restrict__ E, int B) {
  using C = SG<N>;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * N) return;
  const int s = i / N, q = i % N;
  float acc = 0.f;
  for (int t = 0; t < C::NTILE; ++t) acc += epart[((size_t)s * C::NTILE + t) * N + q];
  E[i] = acc;
}

// ----------------------------------------------------------------------------------------- backward
// Reverse pass B of layer l, the adjoint of qubits 8..11 in registers: thread c holds psi AND lambda at
// (h << 8) | c, h = 0..15 (pre-ring order).  psi: S_l with the layer's rotations 8..11 re-applied, or (GEN0, layer 0)
// the product state.  lambda: gathered at the ring images (two coalesced runs, scattered through the one LDS tile into
// pre-ring order and read back), or (FIRST) formed as O(ring(k)) psi(k).  d(theta), d(phi) of qubits 8..11 from that
// pair, RY RZ undone on lambda alone, and lambda stored from the registers in pre-ring tile order, 16 runs of 512
// bytes per wave (GEN0: only its bits-8..11 = 0 part, the only one layer 0's pass A reads).  1 LDS scatter + 1 gather
// and 2 barriers in 39 KB of LDS, four workgroups per CU (launch bounds 4: the register budget that goes with it);
// the backward's three calls at n = 16 716 / 571 / 468 instead of 945 / 942 / 854 us with the adjoint swept over psi's
// and lambda's LDS tiles (profiles/r6_24_*).
// Slab row s*16 + t*(16/NTILE) gets the 8 partials of qubits 8..11 (the other rows of the tile's group get zeros in
// those columns).
template <int N, bool FIRST, bool GEN0>
__global__ void __launch_bounds__(NT, 4) pass_b_bwd(const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ gE, int L, int l, int wgroup,
                                                 const cf* __restrict__ psi, const cf* __restrict__ lin,
                                                 cf* __restrict__ lout, float* __restrict__ slab) {
  using C = SG<N>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);
  float* gq = reinterpret_cast<float*>(smem + 256);       // 16
  float* red = reinterpret_cast<float*>(smem + 320);      // NWV * 8
  cf* tq = reinterpret_cast<cf*>(smem + 512);             // lambda, pre-ring tile order
  float* OL = reinterpret_cast<float*>(tq + 4096);        // (FIRST) observable tables
  float* OH = OL + 256;
  cf* PL = reinterpret_cast<cf*>(OH + 256);               // (GEN0) product tables
  cf* PH = PL + 256;
  cf* ZT = PH + 256;                                      // the 16 RZ undo phases of qubits 8..11
  const int t = blockIdx.x, s = blockIdx.y, c = threadIdx.x;
  // the tile's psi and lambda loads first: in flight across the angle / dL/dE loads and the tables (behind them,
  // a second round trip for wave 0 that the barrier made every wave wait out).  32-bit byte offsets from uniform
  // bases: one VGPR per address instead of a 64-bit pair.
  [[maybe_unused]] cf p[16], lv[16];
  if constexpr (!GEN0) {   // psi = S_l
    const char* src = reinterpret_cast<const char*>(psi + (size_t)s * C::D + ((size_t)t << 12));
#pragma unroll
    for (int h = 0; h < 16; ++h) p[h] = *reinterpret_cast<const cf*>(src + (unsigned)((h << 8) | c) * 8u);
  }
  if constexpr (!FIRST) {   // lambda at the ring images of this tile's pre-ring amplitudes
    const int A0 = ring_fwd_scan<N>(t << 12) >> 12, A1 = ring_fwd_scan<N>((t << 12) | 2048) >> 12;
    const char* ls = reinterpret_cast<const char*>(lin + (size_t)s * C::D);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = threadIdx.x + NT * u;
      lv[u] = *reinterpret_cast<const cf*>(ls + (unsigned)(i | ((i & 2048 ? A1 : A0) << 12)) * 8u);
    }
  }
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  if (FIRST && threadIdx.x < N) gq[threadIdx.x] = gE[(size_t)s * N + threadIdx.x];
  __syncthreads();
  // ZT[h] = prod_b (cos phi_b/2, -+ sin phi_b/2) over qubits 8 + b (+ for bit b = 0)
  if (threadIdx.x < 16) {
    cf z = {1.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float4 tg = trig[8 + b];
      z = cmul(z, cf{tg.z, ((threadIdx.x >> b) & 1) ? -tg.w : tg.w});
    }
    ZT[threadIdx.x] = z;
  }
  if constexpr (FIRST) {   // o(j) = sum_q g_q (1 - 2 bit_q(j)) = OL[j & 255] + OH[j >> 8]
    const int i = threadIdx.x;
    float ol = 0.f, oh = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) ol += ((i >> q) & 1) ? -gq[q] : gq[q];
#pragma unroll
    for (int q = 8; q < N; ++q) oh += ((i >> (q - 8)) & 1) ? -gq[q] : gq[q];
    OL[i] = ol;
    if (i < (1 << (N - 8))) OH[i] = oh;
  }
  if constexpr (GEN0) product_tables<N, NT>(trig, PL, PH, 0);
  cf m[16];
  if constexpr (!FIRST) {   // lambda (loaded at the top, all 16 in flight) -> pre-ring order in LDS
    const int A0 = ring_fwd_scan<N>(t << 12) >> 12, A1 = ring_fwd_scan<N>((t << 12) | 2048) >> 12;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = threadIdx.x + NT * u;
      tq[ring_inv_scan<N>(i | ((i & 2048 ? A1 : A0) << 12)) & 4095] = lv[u];
    }
  }
  __syncthreads();   // (the scatter and the RZ phases; FIRST: the observable tables; GEN0: the product tables)
  if constexpr (GEN0) {
#pragma unroll
    for (int h = 0; h < 16; ++h) p[h] = cmul(PL[c], PH[(t << 4) | h]);
  } else {   // this layer's rotations 8..11 re-applied
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float4 tg = trig[8 + b];
#pragma unroll
      for (int h = 0; h < 16; ++h)
        if (!((h >> b) & 1)) gate_fwd(p[h], p[h | (1 << b)], tg);
    }
  }
#pragma unroll
  for (int h = 0; h < 16; ++h) {
    if constexpr (FIRST) {   // lambda = O psi_final, psi_final(ring(k)) = psi(k)
      const int j = ring_fwd_scan<N>((t << 12) | (h << 8) | c);
      const float o = OL[j & 255] + OH[j >> 8];
      m[h] = {p[h].x * o, p[h].y * o};
    } else {
      m[h] = tq[(h << 8) | c];
    }
  }
  float dth[4], dph[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) dth[b] = dph[b] = 0.f;
  // every d(phi) from the pair as it is (Z_b commutes with the layer's gates on other qubits and with RZ_b), the four
  // RZ undone on both at once (one phase per amplitude), every d(theta) from that pair (J_b commutes with RY on
  // other qubits and its own), then RY undone on lambda alone -- 12 vector operations per pair and bit after the
  // phases, against 36 gate by gate on both states (16-qubit backward 3.58 instead of 3.80 ms, profiles/r6_30_*)
#pragma unroll
  for (int h = 0; h < 16; ++h) {
    const float cc = m[h].x * p[h].y - m[h].y * p[h].x;
#pragma unroll
    for (int b = 0; b < 4; ++b) dph[b] += ((h >> b) & 1) ? -cc : cc;
  }
#pragma unroll
  for (int h = 0; h < 16; ++h) {
    const cf z = ZT[h];
    p[h] = cmul(p[h], z);
    m[h] = cmul(m[h], z);
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int h = 0; h < 16; ++h)
      if (!((h >> b) & 1)) {
        const cf p0 = p[h], p1 = p[h | (1 << b)], l0 = m[h], l1 = m[h | (1 << b)];
        dth[b] += -(l0.x * p1.x + l0.y * p1.y) + (l1.x * p0.x + l1.y * p0.y);
      }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float4 tg = trig[8 + b];
#pragma unroll
    for (int h = 0; h < 16; ++h)
      if (!((h >> b) & 1)) {
        const cf m0 = m[h], m1 = m[h | (1 << b)];
        m[h] = {tg.x * m0.x + tg.y * m1.x, tg.x * m0.y + tg.y * m1.y};
        m[h | (1 << b)] = {tg.x * m1.x - tg.y * m0.x, tg.x * m1.y - tg.y * m0.y};
      }
  }
  // the sums pinned here (sunk past block_sum_vec's barrier they kept every product alive: 249 VGPRs spilled)
#pragma unroll
  for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(dth[b]), "+v"(dph[b]));
  char* lo = reinterpret_cast<char*>(lout + (size_t)s * C::D + ((size_t)t << 12));
  int cs = c;   // (opaque: the psi loads' offsets are not kept live -- spilled -- for these stores)
  asm volatile("" : "+v"(cs));
#pragma unroll
  for (int h = 0; h < (GEN0 ? 1 : 16); ++h)   // (GEN0: only bits 8..11 = 0, the part layer 0's pass A reads)
    *reinterpret_cast<float2*>(lo + (unsigned)((h << 8) | cs) * 8u) = make_float2(m[h].x, m[h].y);
  float v[8];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    v[2 * b] = dth[b];
    v[2 * b + 1] = dph[b];
  }
  float o[8];
  block_sum_vec<8>(v, red, o);
  if (threadIdx.x < 8) {
    constexpr int PER = ROWS / C::NTILE;
    const int P = 2 * N * L;
    const int col = (l * N + 8 + threadIdx.x / 2) * 2 + (threadIdx.x & 1);
    float* row = slab + ((size_t)s * ROWS + t * PER) * P + col;
    row[0] = o[threadIdx.x];
#pragma unroll
    for (int r = 1; r < PER; ++r) row[(size_t)r * P] = 0.f;
  }
}

// Reverse pass A of layer 0 (l = 0; pst is not read).  psi is layer 0's product state with qubits 8..11 back at |0>,
// generated in-kernel; it is zero outside brick 0, so ONE workgroup per sample (blockIdx.x = 0) reads that brick of
// lambda and the other bricks' partials are written zero.  psi and lambda go to two padx LDS images with the pass's RZ
// phases undone and every d(phi) taken on the way; every d(theta) in one read-only pass over them (lds_dtheta).
// Lambda is not undone or stored: nothing reads layer 0's result.
template <int N>
__global__ void __launch_bounds__(SG<N>::NTA, 2) pass_a_bwd0(const float* __restrict__ x, const float* __restrict__ w,
                                                          int L, int l, int wgroup, const cf* __restrict__ pst,
                                                          cf* __restrict__ lst, float* __restrict__ slab) {
  using C = SG<N>;
  constexpr int NTA = C::NTA;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);
  float* red = reinterpret_cast<float*>(smem + 256);      // (NTA / 64) * 2AB floats <= 768 B
  cf* tp = reinterpret_cast<cf*>(smem + 1024);   // (padded images, see padx)
  cf* tq = tp + C::AS + C::AS / 8;
  const int br = blockIdx.x, s = blockIdx.y;
  const int P = 2 * N * L;
  // psi = 0 on bricks 1..15: zero partials
  for (int i = threadIdx.x; i < (ROWS - 1) * 2 * C::AB; i += NTA) {
    const int r = 1 + i / (2 * C::AB), j = i % (2 * C::AB);
    slab[((size_t)s * ROWS + r) * P + (l * N + brick_q(j / 2)) * 2 + (j & 1)] = 0.f;
  }
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  cf* ls = lst + (size_t)s * C::D;
  // the pass's RZ phases as one diagonal: amplitude e (brick order) is multiplied by ZL[e & 255] * ZH[e >> 8] when
  // they are undone (qubit q's factor cos(phi/2) +- i sin(phi/2), + for bit 0) -- after the table barrier below
  cf* ZL = reinterpret_cast<cf*>(smem + 1024 + 2 * sizeof(cf) * (C::AS + C::AS / 8) + sizeof(cf) * 512);
  cf* ZH = ZL + 256;
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += NTA) {
    cf a = {1.f, 0.f};
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const float4 t = trig[b];
      a = cmul(a, cf{t.z, ((i >> b) & 1) ? -t.w : t.w});
    }
    ZL[i] = a;
    if (i < (1 << (C::AB - 8))) {
      cf h = {1.f, 0.f};
#pragma unroll
      for (int b = 8; b < C::AB; ++b) {
        const float4 t = trig[brick_q(b)];
        h = cmul(h, cf{t.z, ((i >> (b - 8)) & 1) ? -t.w : t.w});
      }
      ZH[i] = h;
    }
  }
  // The brick's work stays the body of a rolled loop of ONE trip (as in pass_a_bwd1, which says why), and `take` a
  // lambda: written straight-line, the compiler emits other machine code for this kernel.
#pragma unroll 1
  for (int bi = 0; bi < 1; ++bi) {
    __syncthreads();
    // psi / lambda into the images; every d(phi) of the pass at this point (Im<lam| Z_q |psi>: the RZ of other qubits
    // commute with Z_q), then all the pass's RZ undone at once
    float dz[C::AB];
#pragma unroll
    for (int b = 0; b < C::AB; ++b) dz[b] = 0.f;
    auto take = [&](int e, cf p, cf m) __attribute__((always_inline)) {
      const float c = m.x * p.y - m.y * p.x;
#pragma unroll
      for (int b = 0; b < C::AB; ++b) dz[b] += ((e >> b) & 1) ? -c : c;
      const cf z = cmul(ZL[e & 255], ZH[e >> 8]);
      tp[padx(e)] = cmul(p, z);
      tq[padx(e)] = cmul(m, z);
    };
    cf* PL = tq + C::AS + C::AS / 8;
    cf* PH = PL + 256;
    product_tables<N, NTA>(trig, PL, PH, 0xF00);
    __syncthreads();
    for (int e = threadIdx.x; e < C::AS; e += NTA) {
      const int k = brick_k(e, 0);
      take(e, cmul(PL[k & 255], PH[k >> 8]), ls[k]);
    }
    if (threadIdx.x < (NTA / 64) * 2 * C::AB) red[threadIdx.x] = 0.f;   // (per-wave gradient slots)
    __syncthreads();
    {
      const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
      for (int b = 0; b < C::AB; ++b) {
        const float sz = wave_sum(dz[b]);
        if (lane == 0) red[wv * 2 * C::AB + 2 * b + 1] = sz;
      }
    }
    lds_dtheta<C::AB, C::AB, NTA>(tp, tq, red);
    if (threadIdx.x < 2 * C::AB) {   // (lds_dtheta ended with a barrier: every wave's slot is final)
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < NTA / 64; ++k) o += red[k * 2 * C::AB + threadIdx.x];
      const int q = brick_q(threadIdx.x / 2);
      slab[((size_t)s * ROWS + br) * P + (l * N + q) * 2 + (threadIdx.x & 1)] = o;
    }
  }
}

// Reverse pass A of layers l > 0, one workgroup per (sample, brick), on ONE padq LDS tile: lambda stays in registers in
// its load layout while psi goes through the tile.  d(phi) of every bit and d(theta) of the register bits (bit 0, bits
// RLO..) come from the thread's own loaded pairs; d(theta) of the LDS bits 1 .. RLO - 1 from psi's partner amplitudes
// read in the tile -- for bit b the thread's pairs (2 t, 2 t + 1) + 2 NTA i meet psi at 2 t ^ 2^b, one 16-byte read
// per pair and bit, sign = bit b of 2 t (constant over i).  Then lambda -- its register bits already undone: RY of
// different qubits commute -- takes the tile and is undone group by group (lds_group_lam), the second group storing it
// straight to HBM.  psi is never undone.  ~38 KB of LDS, 89 VGPRs at n = 16: the LDS allows four workgroups per CU;
// launch bounds 3 (4 measured level, profiles/r6_50_*).  Against the same sums over two LDS tiles with the next
// brick's loads held in registers (79 KB, two workgroups per CU): 16-qubit backward 3.10 / 3.12 instead of 3.34 /
// 3.37 ms (profiles/r6_49_*); one brick per workgroup 3.04-3.06 against 3.10-3.11 ms at four
// (profiles/r6_50_qstream_bpb_probe.txt); the second group's stores straight to HBM instead of a read-back in the load
// layout, config 5 4.89-4.90 against 4.92-4.94 ms (profiles/r6_61_qstream_out2_ab.txt).
// The kernel was tuned against spills at n = 16 in a form that walked several bricks, and its shape is kept: the
// brick's work is the body of a rolled loop of ONE trip, the loads and the register undo are lambdas, and the asm
// statements pin what the compiler otherwise moved.  Written straight-line it compiles to other machine code (another
// register allocation), which would need its own measurement.
template <int N>
__global__ void __launch_bounds__(SG<N>::NTA, 3) pass_a_bwd1(const float* __restrict__ x, const float* __restrict__ w,
                                                           int L, int l, int wgroup, const cf* __restrict__ pst,
                                                           cf* __restrict__ lst, float* __restrict__ slab) {
  using C = SG<N>;
  constexpr int NTA = C::NTA, AB = C::AB, AS = C::AS;
  constexpr int NPAIR = AS / (2 * NTA);
  constexpr int RLO = ilog2c(2 * NTA), NRB = 1 + ilog2c(NPAIR);
  constexpr int NB1 = RLO - 1 < 4 ? RLO - 1 : 4, NB2 = RLO - 1 - NB1;
  static_assert(NB2 > 0 && (2 * NTA) % 32 == 0, "two LDS groups; register index strides whole pad blocks");
  constexpr int IST = 2 * NTA + PADQ * ((2 * NTA) / 32);   // tile stride of register index i
  constexpr bool ZSEP = (2 * NTA) % 256 == 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem);
  float* red = reinterpret_cast<float*>(smem + 256);   // (NTA / 64) * 2 AB floats, every slot written
  cf* T = reinterpret_cast<cf*>(smem + 1024);
  cf* ZL = T + AS + PADQ * (AS / 32);
  cf* ZH = ZL + 256;
  const int s = blockIdx.y;
  const int P = 2 * N * L;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  char* lc = reinterpret_cast<char*>(lst + (size_t)s * C::D);
  const char* pc = reinterpret_cast<const char*>(pst + (size_t)s * C::D);
  const int t2 = 2 * threadIdx.x;
  // the brick's psi / lambda pairs (32-bit byte offsets from the sample's uniform bases: one VGPR per address, the
  // 64-bit per-pair addresses kept live to the stores spilled), issued before the angle loads and the tables: in
  // flight across them
  float4 na[NPAIR], nb[NPAIR];
  auto load_brick = [&](int br, int tt) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      const unsigned o = (unsigned)brick_k(tt + 2 * NTA * i, br) * (unsigned)sizeof(cf);
      na[i] = *reinterpret_cast<const float4*>(pc + o);
      nb[i] = *reinterpret_cast<const float4*>(lc + o);
    }
  };
  load_brick(blockIdx.x, t2);
  load_trig<N>(trig, x, w, s, L, l, wgroup);
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += NTA) {   // the pass's RZ diagonal (pass_a_bwd0's tables)
    cf a = {1.f, 0.f};
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const float4 t = trig[b];
      a = cmul(a, cf{t.z, ((i >> b) & 1) ? -t.w : t.w});
    }
    ZL[i] = a;
    if (i < (1 << (AB - 8))) {
      cf h = {1.f, 0.f};
#pragma unroll
      for (int b = 8; b < AB; ++b) {
        const float4 t = trig[brick_q(b)];
        h = cmul(h, cf{t.z, ((i >> (b - 8)) & 1) ? -t.w : t.w});
      }
      ZH[i] = h;
    }
  }
#pragma unroll 1
  for (int bi = 0; bi < 1; ++bi) {   // (one trip: see the kernel's header)
    const int br = blockIdx.x + bi;
    // (the thread's index opaque from here on: the LDS and table addresses derived from it are computed afresh, not
    // shared with the load addresses above -- kept live together, two dozen of them spilled at n = 16)
    int tt = t2;
    asm volatile("" : "+v"(tt));
    const int pbb = padq(tt);
    __syncthreads();   // (the tables)
    asm volatile("" : : : "memory");   // (the RZ factors read from the tables in here: hoisted above, they spilled)
    cf p[2 * NPAIR], m[2 * NPAIR];
    float csum = 0.f, cb[NRB];
#pragma unroll
    for (int b = 0; b < NRB; ++b) cb[b] = 0.f;
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      p[2 * i] = cf{na[i].x, na[i].y};
      m[2 * i] = cf{nb[i].x, nb[i].y};
      p[2 * i + 1] = cf{na[i].z, na[i].w};
      m[2 * i + 1] = cf{nb[i].z, nb[i].w};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * i + h;
        const float c = m[j].x * p[j].y - m[j].y * p[j].x;
        csum += c;
#pragma unroll
        for (int b = 0; b < NRB; ++b) cb[b] += ((j >> b) & 1) ? -c : c;
      }
    }
    asm volatile("" : "+v"(csum));
#pragma unroll
    for (int b = 0; b < NRB; ++b) asm volatile("" : "+v"(cb[b]));
#pragma unroll
    for (int j = 0; j < 2 * NPAIR; ++j) {   // the pass's RZ phases undone on both states
      const int i = j >> 1, h = j & 1;
      const int eh = tt + 2 * NTA * i + h;
      // (2 NTA a multiple of 256: the low factor depends on h only)
      const cf z = ZSEP ? cmul(ZL[(tt + h) & 255], ZH[eh >> 8]) : cmul(ZL[eh & 255], ZH[eh >> 8]);
      p[j] = cmul(p[j], z);
      m[j] = cmul(m[j], z);
    }
    float dthr[NRB];   // d(theta) of the register bits (bit 0, bits RLO ..) from the pair as loaded
#pragma unroll
    for (int b = 0; b < NRB; ++b) {
      dthr[b] = 0.f;
#pragma unroll
      for (int j = 0; j < 2 * NPAIR; ++j)
        if (!((j >> b) & 1)) {
          const cf p0 = p[j], p1 = p[j | (1 << b)], l0 = m[j], l1 = m[j | (1 << b)];
          dthr[b] += -(l0.x * p1.x + l0.y * p1.y) + (l1.x * p0.x + l1.y * p0.y);
        }
    }
    // the sums pinned here: left alone, the compiler sank their adds past the barrier below to the wave reductions,
    // keeping every product alive across the LDS write (spilled at n = 16)
#pragma unroll
    for (int b = 0; b < NRB; ++b) asm volatile("" : "+v"(dthr[b]));
#pragma unroll
    for (int i = 0; i < NPAIR; ++i)   // psi to the tile
      *lds16(T + pbb + i * IST) = make_float4(p[2 * i].x, p[2 * i].y, p[2 * i + 1].x, p[2 * i + 1].y);
    // every d(phi): bit 0 and bits RLO.. by register index, bits 1 .. RLO - 1 by this thread's sign
#pragma unroll
    for (int b = 0; b < AB; ++b) {
      const float dz = b == 0 ? cb[0] : b < RLO ? (((tt >> b) & 1) ? -csum : csum) : cb[b - RLO + 1];
      const float sz = wave_sum(dz);
      if (lane == 0) red[wv * 2 * AB + 2 * b + 1] = sz;
    }
#pragma unroll
    for (int b = 0; b < NRB; ++b) {
      const float st = wave_sum(dthr[b]);
      if (lane == 0) red[wv * 2 * AB + 2 * (b == 0 ? 0 : RLO + b - 1)] = st;
    }
    __syncthreads();   // psi's tile complete
#pragma unroll 1
    for (int b = 1; b < RLO; ++b) {   // d(theta) of the LDS bits: lambda here against psi's partners (rolled: one bit's
                                      // NPAIR reads in flight -- all of them hoisted spilled at n = 16)
      const int qb = padq(tt ^ (1 << b));
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < NPAIR; ++i) {
        const float4 q = *reinterpret_cast<const float4*>(T + qb + i * IST);
        acc += m[2 * i].x * q.x + m[2 * i].y * q.y + m[2 * i + 1].x * q.z + m[2 * i + 1].y * q.w;
      }
      const float st = wave_sum(((tt >> b) & 1) ? acc : -acc);
      if (lane == 0) red[wv * 2 * AB + 2 * b] = st;
    }
    auto undo_reg = [&]() __attribute__((always_inline)) {   // the register bits undone on lambda
#pragma unroll
      for (int b = 0; b < NRB; ++b) {
        const float4 tg = trig[brick_q(b == 0 ? 0 : RLO + b - 1)];
#pragma unroll
        for (int j = 0; j < 2 * NPAIR; ++j)
          if (!((j >> b) & 1)) {
            const cf m0 = m[j], m1 = m[j | (1 << b)];
            m[j] = {tg.x * m0.x + tg.y * m1.x, tg.x * m0.y + tg.y * m1.y};
            m[j | (1 << b)] = {tg.x * m1.x - tg.y * m0.x, tg.x * m1.y - tg.y * m0.y};
          }
      }
    };
    undo_reg();
    __syncthreads();   // every partner read done: lambda takes the tile
#pragma unroll
    for (int i = 0; i < NPAIR; ++i)
      *lds16(T + pbb + i * IST) = make_float4(m[2 * i].x, m[2 * i].y, m[2 * i + 1].x, m[2 * i + 1].y);
    __syncthreads();
    lds_group_lam<AB, 1, NB1, NTA, 1>(T, trig);
    // the second group stores lambda straight to HBM -- runs of 32 amplitudes per register index -- instead of writing
    // the tile back for a read-back in the load layout
    lds_group_lam<AB, 1 + NB1, NB2, NTA, 2>(T, trig, reinterpret_cast<cf*>(lc), br);
    if (threadIdx.x < 2 * AB) {   // (the last group sweep ended with a barrier: every wave's slot is final)
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < NTA / 64; ++k) o += red[k * 2 * AB + threadIdx.x];
      slab[((size_t)s * ROWS + br) * P + (l * N + brick_q(threadIdx.x / 2)) * 2 + (threadIdx.x & 1)] = o;
    }
  }
}

// dx[s][q] = sum over the sample's 16 slab rows of the layer-0 theta column
__global__ void __launch_bounds__(256) reduce_dx(const float* __restrict__ slab, float* __restrict__ dx, int B, int N,
                                                 int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * N) return;
  const int s = i / N, q = i % N;
  float acc = 0.f;
  for (int r = 0; r < ROWS; ++r) acc += slab[((size_t)s * ROWS + r) * P + 2 * q];
  dx[i] = acc;
}

// ------------------------------------------------------------------------------------------ host
// Dynamic LDS bytes per kernel.
template <int N>
struct Smem {
  // pass A forward: the padq image + the RZ tables (37.5 KB at n = 16: four workgroups per CU), + the GEN tables
  static_assert(PADQ <= 2, "the images are sized for at most two pad amplitudes per 32");
  static constexpr size_t A_FWD = 512 + sizeof(cf) * (SG<N>::AS + SG<N>::AS / 16 + 256 + 16);
  static constexpr size_t A_FWD_GEN = A_FWD + sizeof(cf) * 512;
  static constexpr size_t B_FWD = 512 + sizeof(cf) * 4096;
  // pass B backward: lambda's tile + the FIRST / GEN0 / RZ tables (39 KB: four workgroups per CU)
  static constexpr size_t B_BWD = 512 + sizeof(cf) * 4096 + 2048 + sizeof(cf) * (512 + 16);
  // pass_a_bwd0: psi's and lambda's padx images + the product tables + the RZ tables
  static constexpr size_t A_BWD = 1024 + 2 * sizeof(cf) * (SG<N>::AS + SG<N>::AS / 8) + sizeof(cf) * 512 +
                                   sizeof(cf) * (256 + 16);
  // pass_a_bwd1: one padq tile + the RZ tables
  static constexpr size_t A_BWD1 = 1024 + sizeof(cf) * (SG<N>::AS + PADQ * (SG<N>::AS / 32) + 256 + 16);
};
// (the launches' LDS bytes at the two ends of the range, pinned: a change here changes occupancy)
static_assert(Smem<13>::A_FWD == 7040 && Smem<13>::A_FWD_GEN == 11136 && Smem<13>::B_FWD == 33280 &&
                  Smem<13>::B_BWD == 39552 && Smem<13>::A_BWD == 16512 && Smem<13>::A_BWD1 == 7552,
              "LDS bytes at n = 13");
static_assert(Smem<16>::A_FWD == 37504 && Smem<16>::A_FWD_GEN == 41600 && Smem<16>::B_FWD == 33280 &&
                  Smem<16>::B_BWD == 39552 && Smem<16>::A_BWD == 81024 && Smem<16>::A_BWD1 == 38016,
              "LDS bytes at n = 16");

inline size_t state_bytes(int n, int B) { return (size_t)B * (8ull << n); }
inline size_t epart_bytes(int n, int B) { return ((size_t)B * (1ull << (n - 12)) * n * 4 + 255) & ~(size_t)255; }

// Forward.  ws: [T: pass-B outputs][<Z> partials][S: pass-A outputs when psave is null].  psave (nullable):
// L - 1 states, S_l = pass A of layer l's output (the backward's psi).
template <int N>
static int fwd(const float* x, const float* w, float* E, int B, int L, int wgroup, char* ws, cf* psave,
               hipStream_t st) {
  using C = SG<N>;
  using S = Smem<N>;
  const size_t sb = state_bytes(N, B);
  cf* T = reinterpret_cast<cf*>(ws);
  float* epart = reinterpret_cast<float*>(ws + sb);
  cf* S0 = reinterpret_cast<cf*>(ws + sb + epart_bytes(N, B));
  static bool attr = false;
  if (!attr) {
    (void)allow_lds(pass_a_fwd<N, true>, S::A_FWD_GEN);
    (void)allow_lds(pass_a_fwd<N, false>, S::A_FWD);
    (void)allow_lds(pass_b_fwd<N, true>, S::B_FWD);
    (void)allow_lds(pass_b_fwd<N, false>, S::B_FWD);
    attr = true;
  }
  const dim3 ga(ROWS, B), gb(C::NTILE, B);
  for (int l = 1; l < L; ++l) {
    cf* a_out = psave ? reinterpret_cast<cf*>(reinterpret_cast<char*>(psave) + (size_t)(l - 1) * sb) : S0;
    if (l == 1)
      hipLaunchKernelGGL((pass_a_fwd<N, true>), ga, dim3(NT), S::A_FWD_GEN, st, x, w, L, l, wgroup, nullptr, a_out);
    else
      hipLaunchKernelGGL((pass_a_fwd<N, false>), ga, dim3(NT), S::A_FWD, st, x, w, L, l, wgroup, T, a_out);
    if (l == L - 1)
      hipLaunchKernelGGL((pass_b_fwd<N, true>), gb, dim3(NT), S::B_FWD, st, x, w, L, l, wgroup, a_out, nullptr, epart);
    else
      hipLaunchKernelGGL((pass_b_fwd<N, false>), gb, dim3(NT), S::B_FWD, st, x, w, L, l, wgroup, a_out, T, epart);
  }
  if (E) hipLaunchKernelGGL(reduce_e<N>, dim3((B * N + 255) / 256), dim3(256), 0, st, epart, E, B);
  return (int)hipGetLastError();
}

// The forward's passes (as fwd, no state kept) with the probabilities pass in place of the last pass B: probs (B, D)
// fp32, runtot (nullable) (B, D / 2048) uint32.  ws: the forward's workspace.
template <int N>
static int probs_fwd(const float* x, const float* w, float* probs, uint32_t* runtot, int B, int L, int wgroup,
                     char* ws, hipStream_t st) {
  using C = SG<N>;
  using S = Smem<N>;
  const size_t sb = state_bytes(N, B);
  cf* T = reinterpret_cast<cf*>(ws);
  cf* S0 = reinterpret_cast<cf*>(ws + sb + epart_bytes(N, B));
  static bool attr = false;
  if (!attr) {
    (void)allow_lds(pass_a_fwd<N, true>, S::A_FWD_GEN);
    (void)allow_lds(pass_a_fwd<N, false>, S::A_FWD);
    (void)allow_lds(pass_b_fwd<N, false>, S::B_FWD);
    attr = true;
  }
  const dim3 ga(ROWS, B), gb(C::NTILE, B);
  for (int l = 1; l < L; ++l) {
    if (l == 1)
      hipLaunchKernelGGL((pass_a_fwd<N, true>), ga, dim3(NT), S::A_FWD_GEN, st, x, w, L, l, wgroup, nullptr, S0);
    else
      hipLaunchKernelGGL((pass_a_fwd<N, false>), ga, dim3(NT), S::A_FWD, st, x, w, L, l, wgroup, T, S0);
    if (l < L - 1)
      hipLaunchKernelGGL((pass_b_fwd<N, false>), gb, dim3(NT), S::B_FWD, st, x, w, L, l, wgroup, S0, T, nullptr);
    else if (runtot != nullptr)
      hipLaunchKernelGGL((pass_b_probs<N, true>), gb, dim3(NT), S::B_FWD, st, x, w, L, l, wgroup, S0, probs, runtot);
    else
      hipLaunchKernelGGL((pass_b_probs<N, false>), gb, dim3(NT), S::B_FWD, st, x, w, L, l, wgroup, S0, probs, runtot);
  }
  return (int)hipGetLastError();
}

// (csrc/hip/qsim_stream_shots.hip's entry points check the arguments)
int probs_passes(const float* x, const float* w, float* probs, uint32_t* runtot, int B, int n, int L, int wgroup,
                 char* ws, hipStream_t st) {
  switch (n) {
    case 13: return probs_fwd<13>(x, w, probs, runtot, B, L, wgroup, ws, st);
    case 14: return probs_fwd<14>(x, w, probs, runtot, B, L, wgroup, ws, st);
    case 15: return probs_fwd<15>(x, w, probs, runtot, B, L, wgroup, ws, st);
    case 16: return probs_fwd<16>(x, w, probs, runtot, B, L, wgroup, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// Backward.  ws: [lambda 1][lambda 2][forward ws: T, <Z> partials][L - 1 kept states when psave is null].  The whole
// batch in one pass per kernel: run chunk by chunk (the lambda buffers cache-resident) it measured slower at every
// chunk size (profiles/r6_46_*).
template <int N>
static int bwd(const float* x, const float* w, const float* gE, float* dx, float* slab, int B, int L, int wgroup,
               char* ws, cf* psave, hipStream_t st) {
  using C = SG<N>;
  using S = Smem<N>;
  const size_t sb = state_bytes(N, B);
  cf* L1 = reinterpret_cast<cf*>(ws);
  cf* L2 = reinterpret_cast<cf*>(ws + sb);
  if (psave == nullptr) {   // no kept states: run the forward first
    psave = reinterpret_cast<cf*>(ws + 3 * sb + epart_bytes(N, B));
    if (int e = fwd<N>(x, w, nullptr, B, L, wgroup, ws + 2 * sb, psave, st)) return e;
  }
  static bool attr = false;
  if (!attr) {
    (void)allow_lds(pass_b_bwd<N, true, false>, S::B_BWD);
    (void)allow_lds(pass_b_bwd<N, false, false>, S::B_BWD);
    (void)allow_lds(pass_b_bwd<N, false, true>, S::B_BWD);
    (void)allow_lds(pass_a_bwd0<N>, S::A_BWD);
    (void)allow_lds(pass_a_bwd1<N>, S::A_BWD1);
    attr = true;
  }
  const dim3 ga(ROWS, B), gb(C::NTILE, B);
  const cf* lin = nullptr;
  for (int l = L - 1; l >= 0; --l) {
    cf* lo = ((L - 1 - l) % 2 == 0) ? L1 : L2;
    const cf* ps = l > 0 ? reinterpret_cast<const cf*>(reinterpret_cast<const char*>(psave) + (size_t)(l - 1) * sb)
                         : nullptr;
    if (l == L - 1)
      hipLaunchKernelGGL((pass_b_bwd<N, true, false>), gb, dim3(NT), S::B_BWD, st, x, w, gE, L, l, wgroup, ps, lin, lo,
                         slab);
    else if (l > 0)
      hipLaunchKernelGGL((pass_b_bwd<N, false, false>), gb, dim3(NT), S::B_BWD, st, x, w, gE, L, l, wgroup, ps, lin, lo,
                         slab);
    else
      hipLaunchKernelGGL((pass_b_bwd<N, false, true>), gb, dim3(NT), S::B_BWD, st, x, w, gE, L, l, wgroup, ps, lin, lo,
                         slab);
    if (l > 0)
      hipLaunchKernelGGL(pass_a_bwd1<N>, ga, dim3(C::NTA), S::A_BWD1, st, x, w, L, l, wgroup, ps, lo, slab);
    else
      hipLaunchKernelGGL(pass_a_bwd0<N>, dim3(1, B), dim3(C::NTA), S::A_BWD, st, x, w, L, l, wgroup, ps, lo, slab);
    lin = lo;
  }
  hipLaunchKernelGGL(reduce_dx, dim3((B * N + 255) / 256), dim3(256), 0, st, slab, dx, B, N, 2 * N * L);
  return (int)hipGetLastError();
}

}  // namespace qstream
}  // namespace qd

using namespace qd::qstream;

#define QD_STREAM_DISPATCH(n, CALL)         \
  switch (n) {                              \
    case 13: return CALL(13);               \
    case 14: return CALL(14);               \
    case 15: return CALL(15);               \
    case 16: return CALL(16);               \
    default: return (int)hipErrorInvalidValue; \
  }

// Whether (n, L) runs on the streamed simulator (else qsim_big.hip's workgroup-per-sample kernels).
QD_API int qd_qsim_stream_ok(int n, int L) { return n >= 13 && n <= 16 && L >= 2 && 2 * n * L <= 1024; }

// Slab rows of the backward's weight-gradient partials: 16 per sample.
QD_API int qd_qsim_stream_rows(int B) { return B * ROWS; }

// Workspace bytes (see fwd / bwd): forward 2 states + the <Z> partials; backward 3 states + the partials +
// the L - 1 kept states of a forward recompute (used when the caller kept none).
QD_API long long qd_qsim_stream_workspace(int n, int B, int L, int backward) {
  if (n < 13 || n > 16 || B < 1 || L < 2) return 0;
  const long long sb = (long long)state_bytes(n, B), ep = (long long)epart_bytes(n, B);
  return backward ? (3 + (long long)(L - 1)) * sb + ep : 2 * sb + ep;
}

// Bytes of the forward's kept states (psave): L - 1 states of B x 2^n complex64.
QD_API long long qd_qsim_stream_save_bytes(int n, int B, int L) {
  if (n < 13 || n > 16 || B < 1 || L < 2) return 0;
  return (long long)(L - 1) * (long long)state_bytes(n, B);
}

// E (B, n) = <Z>; psave (nullable): qd_qsim_stream_save_bytes of kept states for qd_qsim_stream_bwd.
QD_API int qd_qsim_stream_fwd(const float* x, const float* w, float* E, int B, int n, int L, int wgroup, void* ws,
                              void* psave, void* stream) {
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;   // (G = B / wgroup weight groups, workspace)
  if (!qd_qsim_stream_ok(n, L) || B < 1 || ws == nullptr) return (int)hipErrorInvalidValue;
#define CALL_F(NN) fwd<NN>(x, w, E, B, L, wgroup, (char*)ws, (cf*)psave, (hipStream_t)stream)
  QD_STREAM_DISPATCH(n, CALL_F)
#undef CALL_F
}

// dx (B, n), slab (16 B, 2 n L) weight-gradient partials; psave (nullable) is consumed.
QD_API int qd_qsim_stream_bwd(const float* x, const float* w, const float* gE, float* dx, float* slab, int B, int n,
                              int L, int wgroup, void* ws, void* psave, void* stream) {
  if (wgroup > 0 && B % wgroup != 0) return (int)hipErrorInvalidValue;   // (G = B / wgroup weight groups, workspace)
  if (!qd_qsim_stream_ok(n, L) || B < 1 || ws == nullptr) return (int)hipErrorInvalidValue;
#define CALL_B(NN) bwd<NN>(x, w, gE, dx, slab, B, L, wgroup, (char*)ws, (cf*)psave, (hipStream_t)stream)
  QD_STREAM_DISPATCH(n, CALL_B)
#undef CALL_B
}
