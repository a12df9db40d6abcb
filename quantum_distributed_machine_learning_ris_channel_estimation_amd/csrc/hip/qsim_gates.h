// The QSC circuit's primitives, once, for every simulator kernel (qsim*.hip, qsc.hip): the complex pair, the gate
// convention RZ(phi) RY(theta) per wire, the CNOT ring's basis map, and the QuantumNAT weight-noise hash.  The kernels
// must agree bit for bit (zero-threshold noisy shots = plain shots, on-chip = parameter shift), so a change to the
// convention is made here and nowhere else.
#pragma once
#include "common.h"

namespace qd {

struct cf {
  float x, y;
};
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// f(k): basis-state map of the CNOT ring, CNOT(0,1) first ... CNOT(n-2,n-1), then CNOT(n-1,0); f^-1(k): the same
// self-inverse CNOTs in reverse order.
template <int N>
__device__ __forceinline__ int ring_fwd(int k) {
#pragma unroll
  for (int i = 0; i < N - 1; ++i) k ^= ((k >> i) & 1) << (i + 1);
  k ^= (k >> (N - 1)) & 1;
  return k;
}
template <int N>
__device__ __forceinline__ int ring_inv(int k) {
  k ^= (k >> (N - 1)) & 1;
#pragma unroll
  for (int i = N - 2; i >= 0; --i) k ^= ((k >> i) & 1) << (i + 1);
  return k;
}
// The same two maps in closed form (N <= 16): bit j >= 1 of f(k) is the prefix parity of bits 0..j (a log-step XOR
// scan), bit 0 is k_0 ^ parity(all); f^-1(j): restore bit 0 (= j_0 ^ j_{n-1}), then k_i = j_i ^ j_{i-1}.
// Both forms stay: they compute the same map but compile differently, and each kernel keeps the form it was tuned with.
template <int N>
__device__ __forceinline__ int ring_fwd_scan(int k) {
  int p = k ^ (k << 1);
  p ^= p << 2;
  p ^= p << 4;
  if constexpr (N > 8) p ^= p << 8;
  p &= (1 << N) - 1;
  return (p & ~1) | ((k ^ (p >> (N - 1))) & 1);
}
template <int N>
__device__ __forceinline__ int ring_inv_scan(int j) {
  const int j2 = j ^ ((j >> (N - 1)) & 1);
  return j2 ^ ((j2 << 1) & ((1 << N) - 1));
}

// insert NB zero bits at position P into t
template <int P, int NB>
__device__ __forceinline__ int ins_bits(int t) {
  return ((t >> P) << (P + NB)) | (t & ((1 << P) - 1));
}

// (cos, sin) of theta/2 and (cos, sin) of phi/2 of one layer's qubits, into LDS (xs: the embedding angles, layer 0)
__device__ __forceinline__ void layer_trig(float4* trig, const float* wl, const float* xs, int n) {
  if (threadIdx.x < n) {
    const int q = threadIdx.x;
    float s, c, sp, cp;
    __sincosf(0.5f * (wl[2 * q] + (xs ? xs[q] : 0.f)), &s, &c);
    __sincosf(0.5f * wl[2 * q + 1], &sp, &cp);
    trig[q] = make_float4(c, s, cp, sp);
  }
}

// RZ(phi) RY(theta) on the pair (a0: bit 0, a1: bit 1); t = (cos th/2, sin th/2, cos ph/2, sin ph/2)
__device__ __forceinline__ void gate_fwd(cf& a0, cf& a1, float4 t) {
  const cf t0 = {t.x * a0.x - t.y * a1.x, t.x * a0.y - t.y * a1.y};
  const cf t1 = {t.y * a0.x + t.x * a1.x, t.y * a0.y + t.x * a1.y};
  a0 = cmul(t0, cf{t.z, -t.w});
  a1 = cmul(t1, cf{t.z, t.w});
}

// Adjoint step: given psi and lambda AFTER the gate, add dphi = Im<lam|Z|psi>, undo RZ, add dtheta = Im<lam|Y|psi>,
// undo RY.
__device__ __forceinline__ void gate_adj(cf& p0, cf& p1, cf& l0, cf& l1, float4 t, float& dth, float& dph) {
  dph += (l0.x * p0.y - l0.y * p0.x) - (l1.x * p1.y - l1.y * p1.x);
  p0 = cmul(p0, cf{t.z, t.w});
  l0 = cmul(l0, cf{t.z, t.w});
  p1 = cmul(p1, cf{t.z, -t.w});
  l1 = cmul(l1, cf{t.z, -t.w});
  dth += -(l0.x * p1.x + l0.y * p1.y) + (l1.x * p0.x + l1.y * p0.y);
  const cf q0 = p0, q1 = p1, m0 = l0, m1 = l1;
  p0 = {t.x * q0.x + t.y * q1.x, t.x * q0.y + t.y * q1.y};
  p1 = {t.x * q1.x - t.y * q0.x, t.x * q1.y - t.y * q0.y};
  l0 = {t.x * m0.x + t.y * m1.x, t.x * m0.y + t.y * m1.y};
  l1 = {t.x * m1.x - t.y * m0.x, t.x * m1.y - t.y * m0.y};
}

// Sign of a Pauli frame's Z mask fb on basis state js: -a when popc(fb & js) is odd.
__device__ __forceinline__ cf frame_sign(cf a, int fb, int js) {
  return (__popc(fb & js) & 1) ? cf{-a.x, -a.y} : a;
}

// QuantumNAT weight noise: a standard normal from a counter-based hash of (seed, draw counter, element index) -- no
// RNG state, graph-replay safe.  qsc.hip's draw and qsim_mfma.hip's fused prep write bit-identical noisy weights.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float hash_normal(unsigned long long seed, unsigned long long ctr, unsigned int i) {
  const unsigned long long h = mix64(seed ^ mix64(ctr * 0x100000001b3ull + i));
  const float u1 = ((h >> 40) + 1u) * (1.0f / 16777217.0f);          // (0, 1]
  const float u2 = ((h >> 16) & 0xffffffu) * (1.0f / 16777216.0f);   // [0, 1)
  return sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}

}  // namespace qd
