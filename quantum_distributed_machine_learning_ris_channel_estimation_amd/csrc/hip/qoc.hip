// QOC probabilistic gradient pruning: the device-side update of the parameter-shift mask.
//
// An on-chip QNN pays two circuits per parameter and step.  QOC's pruning accumulates gradient magnitudes for
// `accum` = wa steps with every parameter measured, then for `window` = wp steps measures only K of the P
// parameters, sampled without replacement with probability proportional to the accumulated magnitude.  The mask it
// writes is the `mask` argument of qd_qsim_pshift / qd_qsim_noisy_pshift (0 = the parameter's circuits do not run),
// read from device memory -- so the update sits inside a replayed graph like any other kernel of the step.
//
// State: acc (P fp32), mask (P uint8, all ones at start), step (int64 scalar, 0 at start).  2 <= P <= 4096,
// wa >= 1, wp >= 1, 1 <= K <= P.  qd_qoc_update(grad), with s the value of `step` before the call:
//   1. t = s mod (wa + wp).  t == 0: acc is cleared first.  t < wa: acc[p] += |grad[p]| in fp32; a non-finite
//      entry adds nothing, nor does one that would carry acc[p] past the largest finite fp32 (acc stays finite).
//   2. t' = (s + 1) mod (wa + wp).  t' < wa: mask = all ones.  Else the next step's mask is drawn:
//        m = max_p acc[p];  not m > 0: every weight q_p = 1;  else
//        q_p = (uint32) floor(fdiv_rn(acc[p], m) * 2^20) + 1   (correctly rounded fp32 division; the product is exact)
//      and from here on integers only.  For k = 0 .. K-1:
//        S = sum of q over the parameters not yet chosen (uint64);
//        u = word (k & 3) of the Philox4x32-10 block with counter (0x20000000 | k >> 2, 0, lo32(s+1), hi32(s+1)),
//            key (lo32(seed), hi32(seed));
//        r = floor(u S / 2^32), evaluated as u (S >> 32) + ((u (S & (2^32 - 1))) >> 32) (no 64-bit overflow);
//        chosen: the first unchosen p, ascending, whose running sum of q exceeds r.
//      mask[p] = 1 exactly for the K chosen parameters.
//   3. step = s + 1.
// The host twin is qd_cpu_qoc_update (csrc/cpu/qsim_cpu.cpp): bit-identical acc, mask and step.
//
// One workgroup of one wave: lane i owns the contiguous parameters [i c, (i + 1) c), c = ceil(P / 64) <= 64 -- every
// acc, q and mask entry is written and read by its owner alone, so the kernel has no barrier; the K draws are a
// wave scan of the 64 lane sums (kept in registers) and a walk of at most 64 weights by the lane the draw falls in.
#include "qsim_shots_dev.h"

namespace qd {
namespace qoc {
constexpr int kMaxP = 4096;
constexpr int kMaxWindow = 1 << 20;

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ void __launch_bounds__(64) qoc_update_kernel(float* __restrict__ acc, uint8_t* __restrict__ mask,
                                                        unsigned long long* __restrict__ step,
                                                        const float* __restrict__ grad, int P, int wa, int wp, int K,
                                                        unsigned long long seed) {
  __shared__ uint32_t q[kMaxP];
  const int lane = threadIdx.x;
  const int c = (P + 63) >> 6;
  const int p0 = min(P, lane * c), p1 = min(P, p0 + c);
  const unsigned long long s = *step, period = (unsigned long long)(wa + wp);
  const unsigned long long t = s % period, s1 = s + 1, t1 = s1 % period;
  // 1. accumulate
  float m = 0.f;
  for (int p = p0; p < p1; ++p) {
    float a = t == 0 ? 0.f : acc[p];
    if (t < (unsigned long long)wa) {
      const float g = fabsf(grad[p]), a1 = a + g;
      if (isfinite(g) && isfinite(a1)) a = a1;
      acc[p] = a;
    }
    m = fmaxf(m, a);
  }
  // 2. the next step's mask
  if (t1 < (unsigned long long)wa) {
    for (int p = p0; p < p1; ++p) mask[p] = 1;
  } else {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    unsigned long long mine = 0;   // this lane's sum of q over its unchosen parameters
    for (int p = p0; p < p1; ++p) {
      const uint32_t w = m > 0.f ? (uint32_t)floorf(__fdiv_rn(acc[p], m) * 1048576.f) + 1u : 1u;
      q[p] = w;
      mine += w;
      mask[p] = 0;
    }
    qshots::Philox ph = {{0, 0, 0, 0}};
    for (int k = 0; k < K; ++k) {
      unsigned long long incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = shfl_up64(incl, d);
        if (lane >= d) incl += up;
      }
      const unsigned long long S = ((unsigned long long)__shfl((uint32_t)(incl >> 32), 63) << 32) |
                                   __shfl((uint32_t)incl, 63);
      if ((k & 3) == 0)
        ph = qshots::philox4x32_10(0x20000000u | (uint32_t)(k >> 2), 0u, (uint32_t)s1, (uint32_t)(s1 >> 32),
                                   (uint32_t)seed, (uint32_t)(seed >> 32));
      const unsigned long long u = ph.c[k & 3];
      const unsigned long long r = u * (S >> 32) + ((u * (S & 0xFFFFFFFFull)) >> 32);   // < S
      const unsigned long long excl = incl - mine;
      if (r >= excl && r < incl) {   // exactly one lane (mine > 0 there)
        unsigned long long run = excl;
        for (int p = p0; p < p1; ++p) {
          run += q[p];
          if (run > r) {
            mine -= q[p];
            q[p] = 0;
            mask[p] = 1;
            break;
          }
        }
      }
    }
  }
  // 3. (every lane of the one wave read *step in its first instruction; this store is the kernel's last access to it)
  if (lane == 0) *step = s1;
}
}  // namespace qoc
}  // namespace qd

// One update of the pruner state (see the contract above); grad: P fp32.  Out-of-range arguments: hipErrorInvalidValue,
// nothing launched.
QD_API int qd_qoc_update(float* acc, uint8_t* mask, void* step, const float* grad, int P, int wa, int wp, int K,
                         unsigned long long seed, void* stream) {
  using namespace qd::qoc;
  if (!acc || !mask || !step || !grad || P < 2 || P > kMaxP || wa < 1 || wa > kMaxWindow || wp < 1 ||
      wp > kMaxWindow || K < 1 || K > P)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(qoc_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, mask,
                     (unsigned long long*)step, grad, P, wa, wp, K, seed);
  return (int)hipGetLastError();
}
