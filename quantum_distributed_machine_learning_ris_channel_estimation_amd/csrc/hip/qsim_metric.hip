// Block-diagonal Fubini-Study metric of the QSC circuit (n = 2 .. 12) and the natural-gradient solve on it.
// Parameter p = (l n + q) 2 + k is w[l, q, k]; the metric has 2 L blocks of n x n, one per (layer l, k), per sample:
//   k = 0 (RY):  g_ij = (<Y_i Y_j> - <Y_i><Y_j>) / 4 on the state that enters layer l (l = 0: |0..0>, g = I / 4)
//   k = 1 (RZ):  g_ij = (<Z_i Z_j> - <Z_i><Z_j>) / 4 on the state behind layer l's RY gates
// Both are Z covariances of probabilities p_k: m_i = sum_k p_k z_i(k), C_ij = sum_k p_k z_i(k) z_j(k),
// g = (C - m m^T) / 4.
//
// One 256-thread workgroup per sample walks the circuit once -- or, when that leaves the machine empty, one per
// (sample, layer), each rebuilding the state that enters its layer; both run the same loop over the same inline
// pieces, so a sample's row does not depend on the split.  The state lives in LDS (qsim_shots_dev.h); a second
// buffer takes the basis-changed copy and later the probabilities.  Per layer l:
//   RY block: T[k] = i^popc(k) A[k] (RZ(pi/2) on every wire up to a global phase, exact), then apply_layer with
//             RY(pi/2) on every wire.  RX(pi/2)^+ Z RX(pi/2) = Y and RX(pi/2) = RZ(-pi/2) RY(pi/2) RZ(pi/2); the
//             trailing RZ changes no probability.
//   RZ block: A <- layer l applied to A.  RZ changes no probability either.
// apply_layer / product_state end with the CNOT ring, a permutation j = f(k) of the outcomes: the probability of
// outcome k in front of the ring is that of f(k) behind it, so the probabilities are scattered through f^-1 on their
// way into LDS and the covariance sees the state in front of the ring.
//
// The covariance runs on the matrix cores.  With S (2^n x 16) = [1 | z_0 .. z_{n-1} | 0 ..], S^T diag(p) S is a
// 16 x 16 tile with K = 2^n on v_mfma_f32_16x16x4_f32 (fp32 operands: p is not split); row 0 is m, the rest C.  For
// n >= 5 the three lowest wires are folded out of K on the VALU first: per group of 8 outcomes the Walsh sums P, q_0,
// q_1, q_2, q_01, q_02, q_12 (the probabilities weighted by 1, z_a, z_a z_b of the low wires), 24 additions, leave
// K = 2^n / 8 and the operand rows [P | P z_3 .. P z_{n-1} | q_0 q_1 q_2 | q_01 q_02 q_12] (n + 4 <= 16) against the
// columns [1 | z_3 .. z_{n-1}]: an eighth of the products for the same entries.  Wave v takes the K blocks v, v + 4,
// ..., two accumulators alternating; the four waves' tiles are added in wave order: the launch is deterministic.
// g_ij and g_ji are stored from one value.
//
// qd_qng_solve: per block b, A = gsum_b / B + lam I (gsum: the metric rows summed over the B samples by
// qd_reduce_slab), fp32 Cholesky, two triangular solves, the block's n gradient entries (stride 2) overwritten.
#include "qsim_pshift_dev.h"

namespace qd {
namespace qmetric {
using namespace qd::qpshift;

// LDS carve (bytes): the layer's trig (<= 12 float4) | RY(pi/2)'s trig | the waves' partial tiles (NW x 256 floats)
// | the state | the basis-changed copy, later the probabilities and their folded sums
constexpr int O_TRIGY = 192, O_TILE = 384, O_STATE = O_TILE + NW * 256 * 4;
template <int N>
constexpr size_t smem_bytes() {
  return O_STATE + 2 * sizeof(cf) * (1 << N);
}

constexpr int kFillBlocks = 256;   // fewer samples than this (one workgroup per CU): one workgroup per (sample, layer)

// wires folded out of the products' K dimension
template <int N>
constexpr int fold_bits() {
  return N >= 5 ? 3 : 0;
}

// The Z covariance of the probabilities of S (a state behind a CNOT ring; the covariance is that in front of it) into
// out (n x n, row-major).  Pf: 2 x 2^n floats of LDS (the probabilities, then their folded sums), may alias S.  Every
// thread calls it; ends with a barrier.  COV = false (qd_qsim_metric_nocov, timing only) leaves the matrix products
// out: everything else runs.
template <int N, bool COV>
__device__ __forceinline__ void z_covariance(const cf* S, float* Pf, float* tile, float* __restrict__ out) {
  constexpr int D = 1 << N;
  constexpr int PER = D >= NT ? D / NT : 1;
  constexpr int F = fold_bits<N>(), H = N - F;   // low (folded) and high wires
  constexpr int DH = D >> F;                     // K of the products
  constexpr int M = DH / 4;                      // K blocks of four
  static_assert(F == 0 || F == 3, "the fold below is written for three wires");
  static_assert(1 + H + F + F * (F - 1) / 2 <= 16 && DH >= 4, "the operand rows fit one tile");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float pr[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = threadIdx.x + i * NT;
    if (j < D) pr[i] = prob_of(S[j]);
  }
  __syncthreads();   // every amplitude has been read: Pf may overwrite S
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = threadIdx.x + i * NT;
    if (j < D) Pf[ring_inv_scan<N>(j)] = pr[i];
  }
  __syncthreads();
  // Wf[v DH + kh]: v = 0 the sum P over the group's 8 outcomes, 1 .. 3 weighted by z_0, z_1, z_2, 4 .. 6 by z_0 z_1,
  // z_0 z_2, z_1 z_2 (F = 0: the probabilities themselves)
  float* Wf = F ? Pf + D : Pf;
  if constexpr (F == 3) {
    for (int kh = threadIdx.x; kh < DH; kh += NT) {
      const float4 lo = *reinterpret_cast<const float4*>(Pf + 8 * kh), hi = *reinterpret_cast<const float4*>(Pf + 8 * kh + 4);
      const float s0 = lo.x + lo.y, d0 = lo.x - lo.y, s1 = lo.z + lo.w, d1 = lo.z - lo.w;   // (wire 1 = 0 | 1), wire 2 = 0
      const float s2 = hi.x + hi.y, d2 = hi.x - hi.y, s3 = hi.z + hi.w, d3 = hi.z - hi.w;   // wire 2 = 1
      Wf[0 * DH + kh] = (s0 + s1) + (s2 + s3);
      Wf[1 * DH + kh] = (d0 + d1) + (d2 + d3);
      Wf[2 * DH + kh] = (s0 - s1) + (s2 - s3);
      Wf[3 * DH + kh] = (s0 + s1) - (s2 + s3);
      Wf[4 * DH + kh] = (d0 - d1) + (d2 - d3);
      Wf[5 * DH + kh] = (d0 + d1) - (d2 + d3);
      Wf[6 * DH + kh] = (s0 - s1) - (s2 - s3);
    }
    __syncthreads();
  }
  // this lane's operand row / column i: 0 the all-ones vector, 1 .. H high wire F + i - 1 (both operands), then the
  // low wires' 2 F (F - 1) / 2 + F folded sums (rows only), above that padding
  const int i = lane & 15, kq = lane >> 4;
  const int bit = (i >= 1 && i <= H) ? (1 << (i - 1)) : 0;
  const int wsel = (i > H && i <= H + F + F * (F - 1) / 2) ? (i - H) * DH : 0;
  const float aone = i <= H + F + F * (F - 1) / 2 ? 1.f : 0.f, bone = i <= H ? 1.f : 0.f;
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (COV) {
    constexpr int IT = (M + NW - 1) / NW;   // K blocks per wave
#pragma unroll
    for (int u = 0; u < IT; ++u) {
      const int t = wv + u * NW;
      if (M % NW == 0 || t < M) {   // (wave-uniform)
        const int k = 4 * t + kq;
        const bool neg = (k & bit) != 0;
        f4& acc = (u & 1) ? acc1 : acc0;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Wf[wsel + k] * (neg ? -aone : aone), neg ? -bone : bone, acc, 0, 0, 0);
      }
    }
  } else {
    acc0[0] = Wf[wsel + (lane & (DH - 1))];
  }
  // lane's four results: rows 4 kq + r, column i
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[wv * 256 + (4 * kq + r) * 16 + i] = acc0[r] + acc1[r];
  __syncthreads();
  {
    // wires a <= b of the block; (row, column) of the tile that holds m_w and C_ab
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    if (a <= b && b < N) {
      auto at = [&](int r, int c) {
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < NW; ++u) v += tile[u * 256 + r * 16 + c];
        return v;
      };
      auto mean = [&](int w) { return w < F ? at(H + 1 + w, 0) : at(0, w - F + 1); };
      float c;
      if (a == b)
        c = at(0, 0);
      else if (a >= F)
        c = at(a - F + 1, b - F + 1);
      else if (b >= F)
        c = at(H + 1 + a, b - F + 1);
      else
        c = at(H + 1 + F + a + b - 1, 0);   // pairs (0, 1), (0, 2), (1, 2)
      const float g = 0.25f * (c - mean(a) * mean(b));
      out[a * N + b] = g;
      out[b * N + a] = g;
    }
  }
  __syncthreads();
}

template <int N, bool COV>
__global__ void __launch_bounds__(NT) qsim_metric_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ rows, int L, int split) {
  constexpr int D = 1 << N;
  constexpr int GB = group_bits<N>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* trig = reinterpret_cast<float4*>(smem + O_TRIG);
  float4* trigy = reinterpret_cast<float4*>(smem + O_TRIGY);
  float* tile = reinterpret_cast<float*>(smem + O_TILE);
  cf* A = reinterpret_cast<cf*>(smem + O_STATE);
  cf* T = A + D;
  float* Pf = reinterpret_cast<float*>(T);
  // this workgroup's layers l0 .. l1 - 1 of sample b
  const int b = split ? blockIdx.x / L : blockIdx.x;
  const int l0 = split ? blockIdx.x % L : 0, l1 = split ? l0 + 1 : L;
  const float* xs = x + (size_t)b * N;
  float* row = rows + (size_t)b * 2 * L * N * N;
  if (threadIdx.x < N) trigy[threadIdx.x] = make_float4(0.70710678118654752440f, 0.70710678118654752440f, 1.f, 0.f);
  for (int m = 0; m < l1; ++m) {
    float* blk = row + (size_t)m * 2 * N * N;
    if (m >= l0) {
      if (m == 0) {
        if (threadIdx.x < N * N) blk[threadIdx.x] = (threadIdx.x / N == threadIdx.x % N) ? 0.25f : 0.f;
      } else {
        for (int k = threadIdx.x; k < D; k += NT) {
          const cf a = A[k];
          const int c = __popc(k) & 3;
          T[k] = c == 0 ? a : c == 1 ? cf{-a.y, a.x} : c == 2 ? cf{-a.x, -a.y} : cf{a.y, -a.x};
        }
        __syncthreads();
        apply_layer<N, GB>(T, T, trigy);
        z_covariance<N, COV>(T, Pf, tile, blk);
      }
    }
    layer_trig(trig, w + 2 * N * m, m == 0 ? xs : nullptr, N);
    __syncthreads();
    if (m == 0)
      product_state<N>(A, trig);
    else
      apply_layer<N, GB>(A, A, trig);
    if (m >= l0) z_covariance<N, COV>(A, Pf, tile, blk + N * N);
  }
}

template <int N, bool COV>
static int launch(const float* x, const float* w, float* rows, int B, int L, hipStream_t st) {
  const size_t sm = smem_bytes<N>();
  if (hipError_t e = allow_lds(qsim_metric_kernel<N, COV>, sm)) return (int)e;
  const int split = (B < kFillBlocks && L > 1) ? 1 : 0;
  hipLaunchKernelGGL((qsim_metric_kernel<N, COV>), dim3((unsigned)((long long)B * (split ? L : 1))), dim3(NT), sm, st, x, w,
                     rows, L, split);
  return (int)hipGetLastError();
}

constexpr int kSolveMax = 12;

// One wave per block (l, k): A = gsum / B + lam I in LDS, right-looking Cholesky (lane i owns row i), then lane 0
// solves L y = g and L^T d = y.  A pivot that is not positive (NaN input) leaves the block's gradient as it was.
__global__ void __launch_bounds__(64) qng_solve_kernel(const float* __restrict__ gsum, float rB, float lam,
                                                       float* __restrict__ grad, int n) {
  __shared__ float A[kSolveMax * kSolveMax];
  __shared__ float d[kSolveMax];
  const int blk = blockIdx.x, l = blk >> 1, k = blk & 1, lane = threadIdx.x;
  const float* gs = gsum + (size_t)blk * n * n;
  float* g = grad + (size_t)l * n * 2 + k;
  for (int e = lane; e < n * n; e += 64) A[e] = __fdiv_rn(gs[e], rB) + (e / n == e % n ? lam : 0.f);
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const float p = A[j * n + j];
    if (!(p > 0.f)) return;   // (uniform)
    const float r = __fsqrt_rn(p);
    __syncthreads();
    if (lane >= j && lane < n) A[lane * n + j] = lane == j ? r : __fdiv_rn(A[lane * n + j], r);
    __syncthreads();
    if (lane > j && lane < n) {
      const float lij = A[lane * n + j];
      for (int c = j + 1; c <= lane; ++c) A[lane * n + c] -= lij * A[c * n + j];
    }
    __syncthreads();
  }
  if (lane == 0) {
    for (int i = 0; i < n; ++i) {
      float s = g[2 * i];
      for (int c = 0; c < i; ++c) s -= A[i * n + c] * d[c];
      d[i] = __fdiv_rn(s, A[i * n + i]);
    }
    for (int i = n - 1; i >= 0; --i) {
      float s = d[i];
      for (int c = i + 1; c < n; ++c) s -= A[c * n + i] * d[c];
      d[i] = __fdiv_rn(s, A[i * n + i]);
    }
  }
  __syncthreads();
  if (lane < n) g[2 * lane] = d[lane];
}

}  // namespace qmetric
}  // namespace qd

// rows (B, 2 L n n) fp32: sample b's block (l, k) row-major at ((l 2 + k) n + i) n + j; x (B, n), w (L, n, 2) fp32.
template <bool COV>
static int metric_entry(const float* x, const float* w, float* rows, int B, int n, int L, void* stream) {
  using namespace qd::qshots;
  if (x == nullptr || w == nullptr || rows == nullptr) return (int)hipErrorInvalidValue;
  if (n < 2 || n > kMaxQubits || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if ((long long)B * L > 0x7fffffffll) return (int)hipErrorInvalidValue;
  return dispatch_qubits(n, [&](auto N) { return qd::qmetric::launch<N, COV>(x, w, rows, B, L, (hipStream_t)stream); });
}
QD_API int qd_qsim_metric(const float* x, const float* w, float* rows, int B, int n, int L, void* stream) {
  return metric_entry<true>(x, w, rows, B, n, L, stream);
}
// (timing only, scripts/qng_timing.py) the same launch without the covariance products: the rows are not the metric
QD_API int qd_qsim_metric_nocov(const float* x, const float* w, float* rows, int B, int n, int L, void* stream) {
  return metric_entry<false>(x, w, rows, B, n, L, stream);
}

// grad (L, n, 2) fp32, in place: block (l, k)'s n entries <- (gsum_b / B + lam I)^-1 of them; gsum (2 L, n, n) fp32.
QD_API int qd_qng_solve(const float* gsum, int B, float lam, float* grad, int n, int L, void* stream) {
  if (gsum == nullptr || grad == nullptr) return (int)hipErrorInvalidValue;
  if (n < 2 || n > qd::qmetric::kSolveMax || B < 1 || L < 1) return (int)hipErrorInvalidValue;
  if (!(lam > 0.f && lam <= 3.402823466e+38f)) return (int)hipErrorInvalidValue;   // (NaN and inf fail too)
  hipLaunchKernelGGL(qd::qmetric::qng_solve_kernel, dim3((unsigned)(2 * L)), dim3(64), 0, (hipStream_t)stream, gsum,
                     (float)B, lam, grad, n);
  return (int)hipGetLastError();
}
