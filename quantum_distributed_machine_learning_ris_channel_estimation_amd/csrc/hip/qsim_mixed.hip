// Exact expectation of the noisy QSC device (n = 2 .. 8): the density matrix of the circuit under the Pauli channel
// that qsim_noise.hip samples, taken in expectation -- the limit of that kernel for trajectories, shots -> infinity.
// One 256-thread workgroup per sample (a grid-stride loop over the samples when B exceeds the grid).
//
// Definition (csrc/cpu/qsim_cpu.cpp qd_cpu_qsim_mixed_probs implements the same, gate by gate in complex128):
//   site (l, q, 0), after wire q's fused RZ.RY of layer l:   rho <- (1 - p) rho + (p / 3) (X rho X + Y rho Y + Z rho Z)
//           on wire q, p = thr1[q] / 2^32
//   site (l, q, 1), after CNOT(q, (q+1) mod n) of layer l, in ring order:   rho <- (1 - p) rho + (p / 15) sum P rho P
//           over the 15 non-identity two-qubit Paulis on wires (q, (q+1) mod n), p = thr2[q] / 2^32
//   readout E_i = fma(c_i, sum_k rho_kk z_i(k), d_i),  c_i = 1 - (thr01_i + thr10_i) / 65536,
//           d_i = (thr10_i - thr01_i) / 65536  (exact in fp32: the thresholds have 16 bits)
// The thresholds are the integers the sampling kernels compare against, so a sampler's mean converges to exactly this.
//
// How it runs.  rho[r, c] is entry r | c << n of a 2n-bit vector; a gate is U on bit q and conj(U) on bit n + q.  The
// sum over all four Paulis of P rho P is 2 I (x) tr_q rho, so a one-qubit site is (1 - 4p/3) rho + (2p/3) I (x) tr_q rho
// and a two-qubit site (1 - 16p/15) rho + (4p/15) I (x) tr rho: a thread that owns the 4 entries differing in bits
// (q, n + q) does wire q's rotation and site in one sweep, one that owns the 16 entries of bits (c, t, n + c, n + t) a
// CNOT and its site: 2 n sweeps per layer.  The sweeps run in the order r0 r1 c01 r2 c12 ... c(n-2, n-1) c(n-1, 0)
// (a rotation just before the first CNOT on its wire; it commutes with everything on other wires).
//   n <= 7: rho lives in LDS (128 KiB at n = 7).
//   n = 8:  rho lives in the workgroup's 512 KiB slot of the caller's workspace and is walked in LDS-staged tiles of
//           6 wires (4096 entries, 32 KiB; 16 tiles): as many consecutive sweeps as touch at most 6 wires form a phase,
//           every tile is loaded, swept by the whole phase in LDS and stored once.  The first phase generates its tiles
//           and the last one keeps only the diagonal, so every workspace word read was written in the same launch.
// No workgroup waits on another, there are no atomics, and the reductions run in a fixed order: the result of a row
// does not depend on the batch, the grid or the slot it is computed in.
#include "qsim_gates.h"

namespace qd {
namespace qmixed {

constexpr int NT = 256;
constexpr int kMinQubits = 2, kMaxQubits = 8, kLdsQubits = 7;
constexpr int kTileQubits = 6;       // wires of an LDS tile of the workspace path
constexpr int kMaxSites = 4096;      // 2 n L, as for the sampled noise model
constexpr int kPhaseOps = 64;        // sweeps per trig table
constexpr int kGridCapLds = 2048;    // workgroups of the LDS path
constexpr int kGridCapWs = 256;      // ... of the workspace path: one 512 KiB slot each, 128 MiB at most
// LDS carve (bytes): channel constants (8 float4) | tile index table (64 ushort) | wave sums (4 x 8) | diagonal (256) |
// a phase's trig (64 float4) | rho or its tile
constexpr int O_CHAN = 0, O_LUT = 128, O_RED = 256, O_DIAG = 384, O_TRIG = 1408, O_DATA = 2432;
static_assert(O_DATA % 16 == 0, "the data starts on a 16-byte boundary");

struct Op {
  int l, a, b;   // layer; rotation: wire a; CNOT: control a, target b
  bool cnot;
};
// Sweep o of the circuit, 2 n per layer: r0, then r_k c(k-1, k) for k = 1 .. n-1, then c(n-1, 0).
__device__ __forceinline__ Op decode(int o, int n) {
  const int l = o / (2 * n), j = o - l * 2 * n;
  if (j == 0) return {l, 0, 0, false};
  if (j == 2 * n - 1) return {l, n - 1, 0, true};
  const int k = (j + 1) >> 1;
  return (j & 1) ? Op{l, k, k, false} : Op{l, k - 1, k, true};
}

// t with a zero bit inserted at position pos
__device__ __forceinline__ int ins0(int t, int pos) { return ((t >> pos) << (pos + 1)) | (t & ((1 << pos) - 1)); }
// the low bits of v placed on the set bits of mask, ascending
__device__ __forceinline__ int deposit(int v, int mask) {
  int r = 0, j = 0;
  for (int q = 0; q < kMaxQubits; ++q)
    if ((mask >> q) & 1) r |= ((v >> j++) & 1) << q;
  return r;
}

__device__ __forceinline__ cf mix(cf e, cf s, float a, float k) { return {a * e.x + k * s.x, a * e.y + k * s.y}; }

// Wire q's RZ.RY on rho (T: 4^nl entries, local wires) and its one-qubit site; ch = (1 - 4p/3, 2p/3, ., .).
__device__ __forceinline__ void sweep_rot(cf* T, int nl, int q, float4 tg, float4 ch) {
  const int m0 = 1 << q, m1 = 1 << (nl + q);
  const float4 tc = make_float4(tg.x, tg.y, tg.z, -tg.w);   // conj(U) on the column bit
  for (int t = threadIdx.x; t < (1 << (2 * nl - 2)); t += NT) {
    const int base = ins0(ins0(t, q), nl + q);
    cf e0 = T[base], e1 = T[base | m0], e2 = T[base | m1], e3 = T[base | m0 | m1];
    gate_fwd(e0, e1, tg);
    gate_fwd(e2, e3, tg);
    gate_fwd(e0, e2, tc);
    gate_fwd(e1, e3, tc);
    const cf s = {e0.x + e3.x, e0.y + e3.y};   // tr_q rho
    T[base] = mix(e0, s, ch.x, ch.y);
    T[base | m0] = {ch.x * e1.x, ch.x * e1.y};
    T[base | m1] = {ch.x * e2.x, ch.x * e2.y};
    T[base | m0 | m1] = mix(e3, s, ch.x, ch.y);
  }
  __syncthreads();
}

// CNOT(c, t) on rho and its two-qubit site; ch = (., ., 1 - 16p/15, 4p/15).
__device__ __forceinline__ void sweep_cnot(cf* T, int nl, int c, int t, float4 ch) {
  const int lo = c < t ? c : t, hi = c < t ? t : c;
  const int m[4] = {1 << c, 1 << t, 1 << (nl + c), 1 << (nl + t)};
  for (int i = threadIdx.x; i < (1 << (2 * nl - 4)); i += NT) {
    const int base = ins0(ins0(ins0(ins0(i, lo), hi), nl + lo), nl + hi);
    cf e[16];   // j = row control | row target << 1 | column control << 2 | column target << 3
#pragma unroll
    for (int j = 0; j < 16; ++j)
      e[j] = T[base | ((j & 1) ? m[0] : 0) | ((j & 2) ? m[1] : 0) | ((j & 4) ? m[2] : 0) | ((j & 8) ? m[3] : 0)];
    // tr rho over the two wires (the CNOT permutes the block's diagonal: 5 <-> 15)
    const cf s = {(e[0].x + e[5].x) + (e[10].x + e[15].x), (e[0].y + e[5].y) + (e[10].y + e[15].y)};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const cf v = e[j ^ ((j & 1) << 1) ^ ((j & 4) << 1)];   // rho'[r, c] = rho[f(r), f(c)]
      const bool diag = (j & 3) == (j >> 2);
      T[base | ((j & 1) ? m[0] : 0) | ((j & 2) ? m[1] : 0) | ((j & 4) ? m[2] : 0) | ((j & 8) ? m[3] : 0)] =
          diag ? mix(v, s, ch.z, ch.w) : cf{ch.z * v.x, ch.z * v.y};
    }
  }
  __syncthreads();
}

// WS: n = 8, rho in the workgroup's slot of ws; else rho in LDS.
template <bool WS>
__global__ void __launch_bounds__(NT)
    qsim_mixed_kernel(const float* __restrict__ x, const float* __restrict__ w, const uint32_t* __restrict__ thr1,
                      const uint32_t* __restrict__ thr2, const uint32_t* __restrict__ thr_ro, float* __restrict__ E,
                      float* __restrict__ probs, int B, int n, int L, int wgroup, cf* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* chan = reinterpret_cast<float4*>(smem + O_CHAN);
  uint16_t* lut = reinterpret_cast<uint16_t*>(smem + O_LUT);
  float* red = reinterpret_cast<float*>(smem + O_RED);
  float* diag = reinterpret_cast<float*>(smem + O_DIAG);
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  cf* T = reinterpret_cast<cf*>(smem + O_DATA);
  const int D = 1 << n, total = 2 * n * L;
  const int nl = WS ? kTileQubits : n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  cf* G = WS ? ws + ((size_t)blockIdx.x << (2 * n)) : nullptr;

  if (tid < n) {
    const double p1 = (double)thr1[tid] * (1.0 / 4294967296.0), p2 = (double)thr2[tid] * (1.0 / 4294967296.0);
    chan[tid] = make_float4((float)(1.0 - 4.0 * p1 / 3.0), (float)(2.0 * p1 / 3.0), (float)(1.0 - 16.0 * p2 / 15.0),
                            (float)(4.0 * p2 / 15.0));
  }

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xs = x + (size_t)b * n;
    const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * total : 0);
    if (!WS) {
      for (int i = tid; i < D * D; i += NT) T[i] = {i == 0 ? 1.f : 0.f, 0.f};
    }
    for (int o = 0; o < total;) {
      // ---- the phase: sweeps o .. oe - 1 (block-uniform), on the wires of mask
      int mask = WS ? 0 : D - 1, oe = o;
      while (oe < total && oe - o < kPhaseOps) {
        if (WS) {
          const Op op = decode(oe, n);
          const int m = mask | (1 << op.a) | (1 << op.b);
          if (__popc(m) > kTileQubits) break;
          mask = m;
        }
        ++oe;
      }
      if (WS) {
        for (int q = 0; __popc(mask) < kTileQubits; ++q) mask |= 1 << q;
        if (tid < (1 << kTileQubits)) lut[tid] = (uint16_t)deposit(tid, mask);
      }
      if (tid < oe - o) {
        const Op op = decode(o + tid, n);
        if (!op.cnot) {
          const float* wl = wsmp + 2 * (op.l * n + op.a);
          float s, c, sp, cp;
          __sincosf(0.5f * (wl[0] + (op.l == 0 ? xs[op.a] : 0.f)), &s, &c);
          __sincosf(0.5f * wl[1], &sp, &cp);
          trig[tid] = make_float4(c, s, cp, sp);
        }
      }
      __syncthreads();   // chan, lut, trig and (LDS path) the initial rho are visible
      const bool last = oe == total;
      const int ntiles = WS ? 1 << (2 * (n - kTileQubits)) : 1;
      for (int tile = 0; tile < ntiles; ++tile) {
        int fixr = 0, fixc = 0;
        if (WS) {
          const int out = (D - 1) & ~mask;   // the wires outside the tile: their bits are the tile's id
          fixr = deposit(tile & ((1 << (n - kTileQubits)) - 1), out);
          fixc = deposit(tile >> (n - kTileQubits), out);
          for (int i = tid; i < (1 << (2 * kTileQubits)); i += NT) {
            const int g = (lut[i & 63] | fixr) | ((lut[i >> kTileQubits] | fixc) << n);
            T[i] = o == 0 ? cf{g == 0 ? 1.f : 0.f, 0.f} : G[g];
          }
          __syncthreads();
        }
        for (int k = o; k < oe; ++k) {
          const Op op = decode(k, n);
          const int la = WS ? __popc(mask & ((1 << op.a) - 1)) : op.a;
          const int lb = WS ? __popc(mask & ((1 << op.b) - 1)) : op.b;
          if (op.cnot)
            sweep_cnot(T, nl, la, lb, chan[op.a]);
          else
            sweep_rot(T, nl, la, trig[k - o], chan[op.a]);
        }
        if (WS) {
          if (!last) {
            for (int i = tid; i < (1 << (2 * kTileQubits)); i += NT)
              G[(lut[i & 63] | fixr) | ((lut[i >> kTileQubits] | fixc) << n)] = T[i];
          } else if (fixr == fixc && tid < (1 << kTileQubits)) {
            diag[lut[tid] | fixr] = T[tid | (tid << kTileQubits)].x;
          }
          __syncthreads();   // the tile and lut may be rewritten; the slot's stores are visible to the workgroup
        }
      }
      o = oe;
    }
    if (!WS) {
      if (tid < D) diag[tid] = T[tid | (tid << n)].x;
      __syncthreads();
    }
    // ---- the diagonal -> probs, <Z_i> in a fixed order, readout
    const float p = tid < D ? diag[tid] : 0.f;
    if (probs != nullptr && tid < D) probs[(size_t)b * D + tid] = p;
    for (int i = 0; i < n; ++i) {
      const float v = wave_sum(((tid >> i) & 1) ? -p : p);
      if (lane == 0) red[wv * kMaxQubits + i] = v;
    }
    __syncthreads();
    if (tid < n) {
      const float S = (red[tid] + red[kMaxQubits + tid]) + (red[2 * kMaxQubits + tid] + red[3 * kMaxQubits + tid]);
      const float t01 = (float)thr_ro[2 * tid], t10 = (float)thr_ro[2 * tid + 1];
      E[(size_t)b * n + tid] = __fmaf_rn(1.f - (t01 + t10) * (1.f / 65536.f), S, (t10 - t01) * (1.f / 65536.f));
    }
    __syncthreads();   // diag, red and rho start again
  }
}

static int g_force_grid = 0;   // 0: choose; else the workgroups to launch at most (tests, timing)

static inline bool mixed_ok(int n, int L) {
  return n >= kMinQubits && n <= kMaxQubits && L >= 1 && 2ll * n * L <= kMaxSites;
}
static inline int mixed_grid(int n, int B) {
  const int cap = g_force_grid > 0 ? g_force_grid : (n > kLdsQubits ? kGridCapWs : kGridCapLds);
  return B < cap ? B : cap;
}


// ------------------------------------------------------------------------------------------ the adjoint
// Reverse-mode gradient of sum_j gE_j E_j in one launch: G (B, 2 n L), column (l n + q) 2 + k the derivative by
// w[l, q, k] (k = 0: theta, which in layer 0 is also x_q's; k = 1: phi).  E = tr(Lam rho_K) + const with Lam the real
// diagonal sum_j gE_j c_j Z_j.  The kernel recomputes the forward with the forward's sweeps, keeping all of rho_K, then
// runs the sweeps in reverse order on both arrays (Lam[r, c] stored like rho; <Lam, rho> = Re sum conj(Lam) rho):
//   site:      D = a id + k I (x) tr is self-adjoint and keeps the partial trace (a + 2 k = 1, a + 4 k = 1), so
//              Lam <- D(Lam) is the forward's `mix` and rho <- D^-1(rho) is `mix` with (1 / a, -k / a);
//   CNOT:      a permutation that is its own inverse and commutes with its site: sweep_cnot with either constants;
//   rotation:  dphi = <Lam, (-i/2) [Z_q, rho]>, undo RZ on both, dtheta = <Lam, (-i/2) [Y_q, rho]>, undo RY on both.
// a >= 1/3 (7/15) for p <= 1/2; the launcher's callers refuse larger rates, and a workgroup that meets one writes
// NaN rows instead of dividing by a non-positive a.
//   n <= 6: rho and Lam live in LDS.   n = 7, 8: both live in the workgroup's workspace slot (2 x 8 4^n bytes) and are
//   walked in the forward's 6-wire tiles and phases, one tile of each in LDS; the forward's last phase and the
//   reverse's first are one visit of a tile.  Every workspace word read was written earlier in the same launch.
// A derivative is a sum of one real number per quad: per thread in loop order, within the wave, across the four
// waves, then across the tiles in ascending order (a register of the thread that owns the column).  No atomics, no
// workgroup waits on another; a row of G does not depend on the batch, the grid or the slot.
constexpr int kAdjLdsQubits = 6;
constexpr int A_CHAN = 0, A_ICHAN = 128, A_LUT = 256, A_RED = 384, A_GC = 512, A_DIAG = 640, A_LAM = 1664,
              A_TRIG = 2688, A_WRED = 3712, A_NP = 5760, A_PS = 5776, A_DATA = 13984;
static_assert(A_PS + 2 * (kMaxSites + 2) <= A_DATA && A_DATA % 16 == 0, "the phase table fits; 16-byte data");

__device__ __forceinline__ void ry_inv(cf& a0, cf& a1, float c, float s) {
  const cf q0 = a0, q1 = a1;
  a0 = {c * q0.x + s * q1.x, c * q0.y + s * q1.y};
  a1 = {c * q1.x - s * q0.x, c * q1.y - s * q0.y};
}
__device__ __forceinline__ float rdot(cf a, cf b) { return a.x * b.x + a.y * b.y; }

// The reverse of sweep_rot on rho (T) and Lam (Lm): ch the site's (a, k), ci its inverse's (1 / a, -k / a).  The
// workgroup's partial sums of (dtheta, dphi) go to wred[0 .. 3] and wred[4 .. 7], one per wave.
__device__ __forceinline__ void sweep_rot_adj(cf* T, cf* Lm, int nl, int q, float4 tg, float4 ch, float4 ci,
                                              float* wred) {
  const int m0 = 1 << q, m1 = 1 << (nl + q);
  const cf zi = {tg.z * tg.z - tg.w * tg.w, -2.f * tg.z * tg.w};   // e^{-i phi}
  const cf zc = {zi.x, -zi.y};
  float dth = 0.f, dph = 0.f;
  for (int t = threadIdx.x; t < (1 << (2 * nl - 2)); t += NT) {
    const int base = ins0(ins0(t, q), nl + q);
    cf p0 = T[base], p1 = T[base | m0], p2 = T[base | m1], p3 = T[base | m0 | m1];
    cf l0 = Lm[base], l1 = Lm[base | m0], l2 = Lm[base | m1], l3 = Lm[base | m0 | m1];
    const cf s = {p0.x + p3.x, p0.y + p3.y}, sl = {l0.x + l3.x, l0.y + l3.y};
    p0 = mix(p0, s, ci.x, ci.y);
    p3 = mix(p3, s, ci.x, ci.y);
    p1 = {ci.x * p1.x, ci.x * p1.y};
    p2 = {ci.x * p2.x, ci.x * p2.y};
    l0 = mix(l0, sl, ch.x, ch.y);
    l3 = mix(l3, sl, ch.x, ch.y);
    l1 = {ch.x * l1.x, ch.x * l1.y};
    l2 = {ch.x * l2.x, ch.x * l2.y};
    dph += (l1.y * p1.x - l1.x * p1.y) - (l2.y * p2.x - l2.x * p2.y);
    p1 = cmul(p1, zi);
    p2 = cmul(p2, zc);
    l1 = cmul(l1, zi);
    l2 = cmul(l2, zc);
    dth += rdot(cf{l1.x + l2.x, l1.y + l2.y}, cf{p0.x - p3.x, p0.y - p3.y}) -
           rdot(cf{l0.x - l3.x, l0.y - l3.y}, cf{p1.x + p2.x, p1.y + p2.y});
    ry_inv(p0, p1, tg.x, tg.y);
    ry_inv(p2, p3, tg.x, tg.y);
    ry_inv(p0, p2, tg.x, tg.y);
    ry_inv(p1, p3, tg.x, tg.y);
    ry_inv(l0, l1, tg.x, tg.y);
    ry_inv(l2, l3, tg.x, tg.y);
    ry_inv(l0, l2, tg.x, tg.y);
    ry_inv(l1, l3, tg.x, tg.y);
    T[base] = p0, T[base | m0] = p1, T[base | m1] = p2, T[base | m0 | m1] = p3;
    Lm[base] = l0, Lm[base | m0] = l1, Lm[base | m1] = l2, Lm[base | m0 | m1] = l3;
  }
  dth = wave_sum(0.5f * dth);
  dph = wave_sum(dph);
  if ((threadIdx.x & 63) == 0) {
    wred[threadIdx.x >> 6] = dth;
    wred[4 + (threadIdx.x >> 6)] = dph;
  }
  __syncthreads();
}

// WS: n = 7, 8, rho and Lam in the workgroup's slot of ws; else n <= 6, both in LDS.
template <bool WS>
__global__ void __launch_bounds__(NT)
    qsim_mixed_adjoint_kernel(const float* __restrict__ x, const float* __restrict__ w,
                              const uint32_t* __restrict__ thr1, const uint32_t* __restrict__ thr2,
                              const uint32_t* __restrict__ thr_ro, const float* __restrict__ gE,
                              float* __restrict__ Gout, float* __restrict__ E, int B, int n, int L, int wgroup,
                              cf* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* chan = reinterpret_cast<float4*>(smem + A_CHAN);
  float4* ichan = reinterpret_cast<float4*>(smem + A_ICHAN);
  uint16_t* lut = reinterpret_cast<uint16_t*>(smem + A_LUT);
  float* red = reinterpret_cast<float*>(smem + A_RED);
  float* gc = reinterpret_cast<float*>(smem + A_GC);
  float* diag = reinterpret_cast<float*>(smem + A_DIAG);
  float* lam = reinterpret_cast<float*>(smem + A_LAM);
  float4* trig = reinterpret_cast<float4*>(smem + A_TRIG);
  float* wred = reinterpret_cast<float*>(smem + A_WRED);
  int* np_s = reinterpret_cast<int*>(smem + A_NP);
  uint16_t* ps = reinterpret_cast<uint16_t*>(smem + A_PS);
  const int D = 1 << n, total = 2 * n * L;
  const int nl = WS ? kTileQubits : n;
  const int tile_len = 1 << (2 * nl);
  cf* T = reinterpret_cast<cf*>(smem + A_DATA);
  cf* Lm = T + tile_len;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  cf* Gr = WS ? ws + ((size_t)blockIdx.x << (2 * n + 1)) : nullptr;
  cf* Gl = WS ? Gr + ((size_t)1 << (2 * n)) : nullptr;

  if (tid < n) {
    const double p1 = (double)thr1[tid] * (1.0 / 4294967296.0), p2 = (double)thr2[tid] * (1.0 / 4294967296.0);
    const double a1 = 1.0 - 4.0 * p1 / 3.0, k1 = 2.0 * p1 / 3.0, a2 = 1.0 - 16.0 * p2 / 15.0, k2 = 4.0 * p2 / 15.0;
    chan[tid] = make_float4((float)a1, (float)k1, (float)a2, (float)k2);
    const bool ok = thr1[tid] <= 0x80000000u && thr2[tid] <= 0x80000000u;   // a1 >= 1/3, a2 >= 7/15: never <= 0
    ichan[tid] = ok ? make_float4((float)(1.0 / a1), (float)(-k1 / a1), (float)(1.0 / a2), (float)(-k2 / a2))
                    : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid == 0) {   // the forward's phases: ps[p] .. ps[p + 1] - 1 are the sweeps of phase p
    int np = 0;
    for (int o = 0; o < total;) {
      int mask = 0, oe = o;
      while (oe < total && oe - o < kPhaseOps) {
        if (WS) {
          const Op op = decode(oe, n);
          const int m = mask | (1 << op.a) | (1 << op.b);
          if (__popc(m) > kTileQubits) break;
          mask = m;
        }
        ++oe;
      }
      ps[np++] = (uint16_t)o;
      o = oe;
    }
    ps[np] = (uint16_t)total;
    *np_s = np;
  }
  bool bad = false;   // a rate above 1/2: the site's inverse is not taken
  for (int q = 0; q < n; ++q) bad = bad || thr1[q] > 0x80000000u || thr2[q] > 0x80000000u;
  __syncthreads();
  const int NP = *np_s;

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    if (bad) {
      for (int i = tid; i < total; i += NT) Gout[(size_t)b * total + i] = __int_as_float(0x7fc00000);
      if (E != nullptr && tid < n) E[(size_t)b * n + tid] = __int_as_float(0x7fc00000);
      continue;
    }
    const float* xs = x + (size_t)b * n;
    const float* wsmp = w + (wgroup > 0 ? (size_t)(b / wgroup) * total : 0);
    if (tid < n) {
      const float t01 = (float)thr_ro[2 * tid], t10 = (float)thr_ro[2 * tid + 1];
      gc[tid] = gE[(size_t)b * n + tid] * (1.f - (t01 + t10) * (1.f / 65536.f));
    }
    __syncthreads();
    if (tid < D) {   // Lam_K's diagonal
      float v = 0.f;
      for (int j = 0; j < n; ++j) v += ((tid >> j) & 1) ? -gc[j] : gc[j];
      lam[tid] = v;
    }
    for (int ph = 0; ph < 2 * NP - 1; ++ph) {
      // ---- visit ph: forward phases 0 .. NP - 1, then NP - 2 .. 0 in reverse; visit NP - 1 does both directions
      const int p = ph < NP ? ph : 2 * NP - 2 - ph;
      const int o = ps[p], oe = ps[p + 1];
      const bool fwd = ph < NP, rev = ph >= NP - 1;
      int mask = D - 1;
      if (WS) {
        mask = 0;
        for (int k = o; k < oe; ++k) {
          const Op op = decode(k, n);
          mask |= (1 << op.a) | (1 << op.b);
        }
        for (int q = 0; __popc(mask) < kTileQubits; ++q) mask |= 1 << q;
        if (tid < (1 << kTileQubits)) lut[tid] = (uint16_t)deposit(tid, mask);
      }
      if (tid < oe - o) {
        const Op op = decode(o + tid, n);
        if (!op.cnot) {
          const float* wl = wsmp + 2 * (op.l * n + op.a);
          float s, c, sp, cp;
          __sincosf(0.5f * (wl[0] + (op.l == 0 ? xs[op.a] : 0.f)), &s, &c);
          __sincosf(0.5f * wl[1], &sp, &cp);
          trig[tid] = make_float4(c, s, cp, sp);
        }
      }
      __syncthreads();   // chan, lam, lut and trig are visible
      const int ntiles = WS ? 1 << (2 * (n - kTileQubits)) : 1;
      const bool own = rev && tid < 2 * (oe - o) && !decode(o + (tid >> 1), n).cnot;   // a column of G is this thread's
      float acc = 0.f;
      for (int tile = 0; tile < ntiles; ++tile) {
        int fixr = 0, fixc = 0;
        if (WS) {
          const int out = (D - 1) & ~mask;
          fixr = deposit(tile & ((1 << (n - kTileQubits)) - 1), out);
          fixc = deposit(tile >> (n - kTileQubits), out);
        }
        if (WS || ph == 0 || ph == NP - 1) {
          for (int i = tid; i < tile_len; i += NT) {
            const int r = WS ? (lut[i & 63] | fixr) : (i & (D - 1)), c = WS ? (lut[i >> kTileQubits] | fixc) : (i >> n);
            const int g = r | (c << n);
            if (ph == 0)
              T[i] = {g == 0 ? 1.f : 0.f, 0.f};
            else if (WS)
              T[i] = Gr[g];
            if (ph == NP - 1)
              Lm[i] = {r == c ? lam[r] : 0.f, 0.f};
            else if (WS && ph >= NP)
              Lm[i] = Gl[g];
          }
          __syncthreads();
        }
        if (fwd) {
          for (int k = o; k < oe; ++k) {
            const Op op = decode(k, n);
            const int la = WS ? __popc(mask & ((1 << op.a) - 1)) : op.a;
            const int lb = WS ? __popc(mask & ((1 << op.b) - 1)) : op.b;
            if (op.cnot)
              sweep_cnot(T, nl, la, lb, chan[op.a]);
            else
              sweep_rot(T, nl, la, trig[k - o], chan[op.a]);
          }
        }
        if (ph == NP - 1) {   // rho_K's diagonal, before the reverse sweeps take the tile back
          if (WS) {
            if (fixr == fixc && tid < (1 << kTileQubits)) diag[lut[tid] | fixr] = T[tid | (tid << kTileQubits)].x;
          } else if (tid < D) {
            diag[tid] = T[tid | (tid << n)].x;
          }
          __syncthreads();
        }
        if (rev) {
          for (int k = oe - 1; k >= o; --k) {
            const Op op = decode(k, n);
            const int la = WS ? __popc(mask & ((1 << op.a) - 1)) : op.a;
            const int lb = WS ? __popc(mask & ((1 << op.b) - 1)) : op.b;
            if (op.cnot) {
              sweep_cnot(T, nl, la, lb, ichan[op.a]);
              sweep_cnot(Lm, nl, la, lb, chan[op.a]);
            } else {
              sweep_rot_adj(T, Lm, nl, la, trig[k - o], chan[op.a], ichan[op.a], wred + 8 * (k - o));
            }
          }
          if (own) {
            const float* r4 = wred + 8 * (tid >> 1) + 4 * (tid & 1);
            acc += (r4[0] + r4[1]) + (r4[2] + r4[3]);
          }
        }
        if (WS) {
          if (ph < 2 * NP - 2) {
            for (int i = tid; i < tile_len; i += NT) {
              const int g = (lut[i & 63] | fixr) | ((lut[i >> kTileQubits] | fixc) << n);
              Gr[g] = T[i];
              if (rev) Gl[g] = Lm[i];
            }
          }
          __syncthreads();   // the tiles, lut and wred may be rewritten; the slot's stores are visible to the workgroup
        }
      }
      if (own) {
        const Op op = decode(o + (tid >> 1), n);
        Gout[(size_t)b * total + 2 * (op.l * n + op.a) + (tid & 1)] = acc;
      }
    }
    // ---- the forward's readout, operation for operation
    const float pk = tid < D ? diag[tid] : 0.f;
    for (int i = 0; i < n; ++i) {
      const float v = wave_sum(((tid >> i) & 1) ? -pk : pk);
      if (lane == 0) red[wv * kMaxQubits + i] = v;
    }
    __syncthreads();
    if (E != nullptr && tid < n) {
      const float S = (red[tid] + red[kMaxQubits + tid]) + (red[2 * kMaxQubits + tid] + red[3 * kMaxQubits + tid]);
      const float t01 = (float)thr_ro[2 * tid], t10 = (float)thr_ro[2 * tid + 1];
      E[(size_t)b * n + tid] = __fmaf_rn(1.f - (t01 + t10) * (1.f / 65536.f), S, (t10 - t01) * (1.f / 65536.f));
    }
    __syncthreads();   // diag, red, gc, lam and the arrays start again
  }
}

static inline bool adjoint_ws(int n) { return n > kAdjLdsQubits; }
static inline int adjoint_grid(int n, int B) {
  const int cap = g_force_grid > 0 ? g_force_grid : (adjoint_ws(n) ? kGridCapWs : kGridCapLds);
  return B < cap ? B : cap;
}

}  // namespace qmixed
}  // namespace qd

using namespace qd::qmixed;

// (n, L) is in the simulator's range.
QD_API int qd_qsim_mixed_ok(int n, int L) { return mixed_ok(n, L) ? 1 : 0; }

// Bytes of workspace qd_qsim_mixed_fwd needs for a batch of B: one 512 KiB slot per workgroup at n = 8 (sized by the
// grid, not by B), none below.  Ask after qd_qsim_mixed_force_grid, not before.
QD_API long long qd_qsim_mixed_workspace(int n, int B) {
  if (n <= kLdsQubits || n > kMaxQubits || B < 1) return 0;
  return (long long)mixed_grid(n, B) * ((long long)sizeof(qd::cf) << (2 * n));
}

// E (B, n) fp32, and probs (nullable; B, 2^n) fp32: the diagonal of rho before the readout, natural basis order.
// thr1 / thr2 (n) uint32 gate thresholds, thr_ro (n, 2) uint32 readout thresholds (<= 65535): NoiseModel.thresholds.
// w (L, n, 2), or grouped (B / wgroup, L, n, 2) with wgroup > 0.  ws: qd_qsim_mixed_workspace(n, B) bytes (n = 8).
QD_API int qd_qsim_mixed_fwd(const float* x, const float* w, const void* thr1, const void* thr2, const void* thr_ro,
                             float* E, float* probs, int B, int n, int L, int wgroup, void* ws, void* stream) {
  if (!mixed_ok(n, L) || B < 1 || wgroup < 0 || (wgroup > 0 && B % wgroup != 0)) return (int)hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || thr1 == nullptr || thr2 == nullptr || thr_ro == nullptr || E == nullptr)
    return (int)hipErrorInvalidValue;
  const bool use_ws = n > kLdsQubits;
  if (use_ws && ws == nullptr) return (int)hipErrorInvalidValue;
  const int grid = mixed_grid(n, B);
  const size_t sm = O_DATA + (sizeof(qd::cf) << (2 * (use_ws ? kTileQubits : n)));
  const hipStream_t st = (hipStream_t)stream;
  if (use_ws) {
    hipLaunchKernelGGL(qsim_mixed_kernel<true>, dim3(grid), dim3(NT), sm, st, x, w, (const uint32_t*)thr1,
                       (const uint32_t*)thr2, (const uint32_t*)thr_ro, E, probs, B, n, L, wgroup, (qd::cf*)ws);
  } else {
    if (hipError_t e = qd::allow_lds(qsim_mixed_kernel<false>, sm)) return (int)e;
    hipLaunchKernelGGL(qsim_mixed_kernel<false>, dim3(grid), dim3(NT), sm, st, x, w, (const uint32_t*)thr1,
                       (const uint32_t*)thr2, (const uint32_t*)thr_ro, E, probs, B, n, L, wgroup, (qd::cf*)nullptr);
  }
  return (int)hipGetLastError();
}

// Tests and timing: launch at most g workgroups from now on (0 hands the choice back).  At n = 8 the workspace is
// sized by the grid: ask qd_qsim_mixed_workspace again after a change.
QD_API int qd_qsim_mixed_force_grid(int g) {
  if (g < 0 || g > kGridCapLds) return (int)hipErrorInvalidValue;
  g_force_grid = g;
  return 0;
}

// Bytes of workspace qd_qsim_mixed_adjoint needs for a batch of B: rho and Lam, 2 x 8 4^n bytes per workgroup at
// n = 7, 8 (sized by the grid, not by B), none below.  Ask after qd_qsim_mixed_force_grid, not before.
QD_API long long qd_qsim_mixed_adjoint_workspace(int n, int B) {
  if (!adjoint_ws(n) || n > kMaxQubits || B < 1) return 0;
  return (long long)adjoint_grid(n, B) * ((long long)(2 * sizeof(qd::cf)) << (2 * n));
}

// G (B, 2 n L) fp32: row b the gradient of sum_j gE[b, j] E[b, j] by the circuit's parameters, column
// (l n + q) 2 + k for w[l, q, k] (layer 0's k = 0 columns are also x's); every column is written.  E_out (nullable;
// B, n): qd_qsim_mixed_fwd's E, bit for bit.  The other arguments are qd_qsim_mixed_fwd's; the thresholds must not
// exceed 2^31 (p <= 1/2: callers check the host copies they have; a workgroup that meets a larger one writes NaN).
// ws: qd_qsim_mixed_adjoint_workspace(n, B) bytes (n = 7, 8).
QD_API int qd_qsim_mixed_adjoint(const float* x, const float* w, const void* thr1, const void* thr2,
                                 const void* thr_ro, const float* gE, float* G, float* E_out, int B, int n, int L,
                                 int wgroup, void* ws, void* stream) {
  if (!mixed_ok(n, L) || B < 1 || wgroup < 0 || (wgroup > 0 && B % wgroup != 0)) return (int)hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || thr1 == nullptr || thr2 == nullptr || thr_ro == nullptr || gE == nullptr ||
      G == nullptr)
    return (int)hipErrorInvalidValue;
  const bool use_ws = adjoint_ws(n);
  if (use_ws && ws == nullptr) return (int)hipErrorInvalidValue;
  const int grid = adjoint_grid(n, B);
  const size_t sm = A_DATA + ((2 * sizeof(qd::cf)) << (2 * (use_ws ? kTileQubits : n)));
  const hipStream_t st = (hipStream_t)stream;
  if (use_ws) {
    if (hipError_t e = qd::allow_lds(qsim_mixed_adjoint_kernel<true>, sm)) return (int)e;
    hipLaunchKernelGGL(qsim_mixed_adjoint_kernel<true>, dim3(grid), dim3(NT), sm, st, x, w, (const uint32_t*)thr1,
                       (const uint32_t*)thr2, (const uint32_t*)thr_ro, gE, G, E_out, B, n, L, wgroup, (qd::cf*)ws);
  } else {
    if (hipError_t e = qd::allow_lds(qsim_mixed_adjoint_kernel<false>, sm)) return (int)e;
    hipLaunchKernelGGL(qsim_mixed_adjoint_kernel<false>, dim3(grid), dim3(NT), sm, st, x, w, (const uint32_t*)thr1,
                       (const uint32_t*)thr2, (const uint32_t*)thr_ro, gE, G, E_out, B, n, L, wgroup,
                       (qd::cf*)nullptr);
  }
  return (int)hipGetLastError();
}
