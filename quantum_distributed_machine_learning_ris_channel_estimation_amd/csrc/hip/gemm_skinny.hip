// The skinny FC forward: Y[M, N] = A[rows, K] . W[N, K]^T with 1 <= M <= 16 output rows, for the low-latency
// estimate path (train/infer.py InferSession: one pilot frame of 1-16 users, not a sweep chunk).  At these M the
// product is a weight stream: 2048 x 4096 bf16 = 16.8 MB (e4m3: 8.4 MB) read once, against at most 48 operand rows.
// csrc/hip/gemm.hip's 144-row tiles would put 16 workgroups on the chip, each walking the whole K.
//
// Decomposition.  The MFMA is mfma_f32_16x16x32_bf16 (e4m3: mfma_f32_16x16x32_fp8_fp8) with W as its 16-row
// operand and the <= 16 operand rows of A as its 16 columns, so one accumulator tile is 16 output channels x all M
// rows.  A wave owns one column group (16 channels) over a K slice of WS = 64 NC elements; the 4 waves of a
// workgroup take interleaved 64-element chunks of the same column group (chunk c of wave w starts at
// (4 c + w) 64: at any time the workgroup reads 256 contiguous k of its 16 weight rows).  The grid is
// (N / 16) x KS workgroups, KS = K / (4 WS), blockIdx = ks (N / 16) + group:
//     WS = the largest of 512, 256, 128, 64 with K % (4 WS) == 0 and K / (4 WS) >= 2
//     N = 2048, K = 4096: WS 512, KS 2, 256 workgroups (one per CU);  K = 8192: KS 4, 512 workgroups (two per CU)
// Every element of W is read by exactly one wave.  The weights go straight from global memory to the MFMA operand
// registers (16-byte loads: lane (r, g) reads row r, k = 8 g .. 8 g + 7 of a 32-k step -- the e4m3 form 16 k, which
// feed two MFMAs), the whole slice issued before the first MFMA: no LDS stage, nothing shared between waves.  The
// operand rows' K slice comes through L2 the same way; the lanes of the rows >= M repeat row 0's addresses (no line
// that row 0 does not fetch anyway) and their accumulator columns are dropped.
//
// Reduction (fixed order, no float atomics).  The 4 waves' accumulators are summed through LDS as
// ((w0 + w1) + w2) + w3 and the workgroup stores that partial tile to its slab; the workgroup that draws the last
// ticket of its column group sums the KS slabs in slice order 0, 1, .. and runs the epilogue.  The hand-off is the
// counter form: plain slab stores, vmcnt(0), barrier, agent-scope release, relaxed agent-scope fetch_add; the
// last arriver takes an agent-scope acquire before it reads.  Nothing waits on anything, so no workgroup placement
// or dispatch order can hang it.  The last arriver also stores 0 to its ticket, and every slab word that is read was
// written in the same launch: a call leaves the workspace as it found it (tickets zero), and a captured graph
// replays any number of times.  The workspace must start zeroed in its ticket words
// (qd_gemm_fwd_skinny_ws_bytes; ops/fc.py allocates it with torch.zeros) and belongs to one stream at a time.
//
// Row independence.  WS, KS, the chunk order and both summation orders depend on (N, K) only.  Column m of the MFMA
// depends on column m of its operand only, so output row i is the same bits for every M, every other row's operands
// and every other row's expert / weights.
//
// Epilogues: csrc/hip/gemm.hip's, on the reduced accumulator acc[i, j]:
//   routed bf16   bf16(acc + b)                                       (qd_gemm_fwd_bias)
//   mix bf16      bf16(fma(p2, acc2, fma(p1, acc1, p0 acc0)) + b)     (EPI_MIX)
//   routed e4m3   bf16(fma(acc, rs cs, b))                            (qd_gemm_fwd_rows_f8)
//   mix e4m3      p'_e = p_e rs_e, bf16(fma(fma(p'_2, acc2, fma(p'_1, acc1, p'_0 acc0)), cs, b))
// One-hot weights return the selected accumulator unchanged, i.e. the routed call bit for bit.
//
// Rules (qd_gemm_fwd_skinny_ok; anything else: hipErrorInvalidValue before any launch, Y untouched):
//   1 <= M <= 16;  N % 16 == 0, 16 <= N <= 16384;  K % 512 == 0, 512 <= K <= 65536;  mix: E == 3;
//   routed: 1 <= E <= 64, expert required unless E == 1 (values are clamped to [0, E - 1])
//
// Resources (hipcc --offload-arch=gfx950 -O3, NC = 8; VGPRs + accumulator AGPRs): routed bf16 144 + 4, mix bf16
// 188 + 12, routed e4m3 84 + 4, mix e4m3 112 + 12; no scratch; LDS 4.1 KiB (mix: 12.3 KiB).  256 threads (one wave per
// SIMD), so 2 (mix bf16) to 5 (routed e4m3) workgroups fit a CU; the grid puts 1 (K = 4096) or 2 (K = 8192) there.
#include "common.h"

namespace qd {
namespace skinny {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) long l2;

constexpr int kMaxM = 16, kMaxN = 16384, kMaxK = 65536;
// workspace: kMaxN / 16 ticket words, 16 int64 zeros (the expert indices of a call without any), then the slabs
constexpr int kTickBytes = 4096, kHeadBytes = kTickBytes + 256;

struct Args {
  const uint8_t* A;       // operand rows (bf16 or e4m3), row-major, K elements per row
  const uint8_t* W;       // (N, K) weights in the same format
  const uint16_t* bias;   // (N,) bf16, nullable
  const long* expert;     // routed: (M,) (E == 1 without indices: the workspace's zeros)
  const float* P;         // mix: (M, 3)
  const float* rs;        // e4m3: per operand row
  const float* cs;        // e4m3: per output channel
  uint16_t* Y;            // (M, N) bf16
  unsigned int* tick;     // (N / 16) ticket words, zero between calls
  f32x4* slab;            // (KS, N / 16, NE, 64) partial tiles
  int M, N, K, E, KS;
};

// wave slice length in 64-element chunks: 8, 4, 2 or 1 (0: K outside the rules)
static int wave_chunks(int K) {
  if (K < 512 || K > kMaxK || K % 512) return 0;
  for (int nc = 8; nc >= 1; nc >>= 1)
    if (K % (256 * nc) == 0 && K / (256 * nc) >= 2) return nc;
  return 0;
}

template <bool F8, bool MIX, int NC>
__global__ __launch_bounds__(256) void skinny_kernel(const Args a) {
  constexpr int NE = MIX ? 3 : 1;    // operand rows per output row that enter the product
  constexpr int EB = F8 ? 1 : 2;     // bytes per element
  constexpr int NL = F8 ? 1 : 2;     // 16-byte loads per lane and 64-element chunk
  __shared__ f32x4 sm[4 * NE * 64 + 1];   // the waves' accumulators; the last word: "this workgroup reduces"
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, g = lane >> 4;   // weight row / output row of the lane's operands, its k group
  const int ng = a.N >> 4;
  const int grp = blockIdx.x % ng, ks = blockIdx.x / ng;
  const int n0 = grp << 4;
  const size_t kwg = (size_t)ks * (256 * NC);   // the workgroup's K slice starts here
  const bool valid = r < a.M;
  const int rr = valid ? r : 0;   // the lanes of the rows >= M repeat row 0's loads (the same lines; results dropped)

  // the routed row's expert (the oldest load: the weight stream below is not waited for to get it)
  [[maybe_unused]] long x = 0;
  if constexpr (!MIX) {
    x = a.expert[rr];
    x = x < 0 ? 0 : x >= a.E ? a.E - 1 : x;
  }

  // operand rows: routed i E + expert[i] (clamped), mix 3 i + e.  Straight-line loads, no predication (a branch per
  // load would drain the weight stream, vmcnt(0), once per MFMA), in batches of CB chunks: all of them for the routed
  // forms, half for the mix (3 rows per lane: 96 VGPRs a batch at NC = 8)
  constexpr int CB = MIX ? (NC >= 2 ? NC / 2 : 1) : NC;
  const uint8_t* ap[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const size_t row = MIX ? (size_t)3 * rr + e : (size_t)rr * a.E + (size_t)x;
    ap[e] = a.A + (row * a.K + kwg + (F8 ? 16 : 8) * g) * EB;
  }
  u32x4 av[CB][NL][NE];
  auto load_a = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CB; ++c) {
#pragma unroll
      for (int j = 0; j < NL; ++j) {
#pragma unroll
        for (int e = 0; e < NE; ++e)
          av[c][j][e] = *reinterpret_cast<const u32x4*>(ap[e] + (size_t)((4 * (c0 + c) + wave) * 64 + 32 * j) * EB);
      }
    }
  };
  // Issue order (the scheduling barriers keep it: left alone, the compiler trades loads in flight for registers and
  // waits after every MFMA).  Mix: the first operand batch (L2 hits, returned first), then the whole weight slice.
  // Routed: the weight slice at once, then the operand rows, whose addresses wait for the expert index only.
  if constexpr (MIX) {
    load_a(0);
    __builtin_amdgcn_sched_barrier(0);
  }
  const uint8_t* wp = a.W + ((size_t)(n0 + r) * a.K + kwg + (F8 ? 16 : 8) * g) * EB;
  u32x4 w[NC][NL];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int j = 0; j < NL; ++j)
      w[c][j] = *reinterpret_cast<const u32x4*>(wp + (size_t)((4 * c + wave) * 64 + 32 * j) * EB);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (!MIX) {
    load_a(0);
    __builtin_amdgcn_sched_barrier(0);
  }

  f32x4 acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += CB) {
    if (c0 > 0) {
      load_a(c0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
#pragma unroll
      for (int j = 0; j < NL; ++j) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          if constexpr (F8) {
            const l2 wv = __builtin_bit_cast(l2, w[c0 + c][j]), xv = __builtin_bit_cast(l2, av[c][j][e]);
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv.x, xv.x, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv.y, xv.y, acc[e], 0, 0, 0);
          } else {
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w[c0 + c][j]),
                                                             __builtin_bit_cast(bf16x8, av[c][j][e]), acc[e], 0, 0, 0);
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // lane (r, g) now holds output row r, channels n0 + 4 g .. 4 g + 3

  // the 4 waves' partial tiles -> one, in wave order; wave 0 stores it to the slice's slab
#pragma unroll
  for (int e = 0; e < NE; ++e) sm[(wave * NE + e) * 64 + lane] = acc[e];
  __syncthreads();
  f32x4* const slab0 = a.slab + ((size_t)grp * NE) * 64 + lane;
  const size_t slab_ks = (size_t)ng * NE * 64;
  if (wave == 0) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      f32x4 s = sm[e * 64 + lane];
#pragma unroll
      for (int v = 1; v < 4; ++v) s += sm[(v * NE + e) * 64 + lane];
      slab0[ks * slab_ks + e * 64] = s;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned int* const last = reinterpret_cast<unsigned int*>(&sm[4 * NE * 64]);
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(a.tick + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool is_last = t == (unsigned int)(a.KS - 1);
    if (is_last) __hip_atomic_store(a.tick + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call's 0
    *last = is_last;
  }
  __syncthreads();
  if (*last == 0u || wave != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // the column group's KS slabs in slice order, then the epilogue of the lane's 4 channels of row r
  f32x4 s[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) s[e] = slab0[e * 64];
  for (int k = 1; k < a.KS; ++k) {
#pragma unroll
    for (int e = 0; e < NE; ++e) s[e] += slab0[k * slab_ks + e * 64];
  }
  if (!valid) return;
  const int n = n0 + 4 * g;
  [[maybe_unused]] float p[NE];
  if constexpr (MIX) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      p[e] = a.P[3 * r + e];
      if constexpr (F8) p[e] *= a.rs[3 * r + e];   // (a power of two: exact)
    }
  } else if constexpr (F8) {
    p[0] = a.rs[(size_t)r * a.E + (size_t)x];
  }
  float y[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float b = a.bias ? bf16_to_f32(a.bias[n + v]) : 0.f;
    if constexpr (MIX) {
      const float m = __builtin_fmaf(p[2], s[2][v], __builtin_fmaf(p[1], s[1][v], rounded_product(p[0], s[0][v])));
      if constexpr (F8) y[v] = __builtin_fmaf(m, a.cs[n + v], b);
      else y[v] = m + b;
    } else if constexpr (F8) {
      y[v] = __builtin_fmaf(s[0][v], rounded_product(p[0], a.cs[n + v]), b);
    } else {
      y[v] = s[0][v] + b;
    }
  }
  uint2 o;
  o.x = (uint32_t)f32_to_bf16(y[0]) | ((uint32_t)f32_to_bf16(y[1]) << 16);
  o.y = (uint32_t)f32_to_bf16(y[2]) | ((uint32_t)f32_to_bf16(y[3]) << 16);
  *reinterpret_cast<uint2*>(a.Y + (size_t)r * a.N + n) = o;
}

template <bool F8, bool MIX>
static int launch(Args a, void* ws, hipStream_t st) {
  const int nc = wave_chunks(a.K);
  if (nc == 0 || ws == nullptr || !a.A || !a.W || !a.Y) return (int)hipErrorInvalidValue;
  if (a.M < 1 || a.M > kMaxM || a.N < 16 || a.N > kMaxN || a.N % 16) return (int)hipErrorInvalidValue;
  a.KS = a.K / (256 * nc);
  a.tick = reinterpret_cast<unsigned int*>(ws);
  a.slab = reinterpret_cast<f32x4*>(reinterpret_cast<uint8_t*>(ws) + kHeadBytes);
  if (a.expert == nullptr) a.expert = reinterpret_cast<const long*>(reinterpret_cast<uint8_t*>(ws) + kTickBytes);
  const dim3 grid((a.N / 16) * a.KS), block(256);
  if (nc == 8) hipLaunchKernelGGL((skinny_kernel<F8, MIX, 8>), grid, block, 0, st, a);
  else if (nc == 4) hipLaunchKernelGGL((skinny_kernel<F8, MIX, 4>), grid, block, 0, st, a);
  else if (nc == 2) hipLaunchKernelGGL((skinny_kernel<F8, MIX, 2>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((skinny_kernel<F8, MIX, 1>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace skinny
}  // namespace qd

using qd::skinny::Args;

// Do the skinny forwards cover (M, N, K)?  (One rule set for bf16 and e4m3: a 16-byte load is one 64-element chunk of
// an e4m3 row, half of one of a bf16 row.)
QD_API int qd_gemm_fwd_skinny_ok(int M, int N, int K, int fp8) {
  (void)fp8;
  return M >= 1 && M <= qd::skinny::kMaxM && N >= 16 && N <= qd::skinny::kMaxN && N % 16 == 0 &&
         qd::skinny::wave_chunks(K) != 0;
}

// Bytes of the workspace for (N, K), any M and any of the four forms (0: outside the rules): the ticket words and 16
// zero indices, then KS (N / 16) 3 partial tiles of 1 KiB.  Zero it once; every call leaves it zeroed where that matters.
QD_API long qd_gemm_fwd_skinny_ws_bytes(int N, int K) {
  const int nc = qd::skinny::wave_chunks(K);
  if (nc == 0 || N < 16 || N > qd::skinny::kMaxN || N % 16) return 0;
  return qd::skinny::kHeadBytes + (long)(K / (256 * nc)) * (N / 16) * 3 * 1024;
}

// Y (M, N) bf16 = bf16(A[i E + expert[i]] . W^T + bias): qd_gemm_fwd_bias's routed rows for 1 <= M <= 16.
QD_API int qd_gemm_fwd_skinny(const uint16_t* A, const uint16_t* W, const uint16_t* bias, uint16_t* Y, int M, int N,
                              int K, const long* expert, int E, void* ws, void* stream) {
  if (E < 1 || E > 64 || (expert == nullptr && E != 1)) return (int)hipErrorInvalidValue;
  Args a{reinterpret_cast<const uint8_t*>(A), reinterpret_cast<const uint8_t*>(W), bias, expert, nullptr, nullptr,
         nullptr, Y, nullptr, nullptr, M, N, K, E, 0};
  return qd::skinny::launch<false, false>(a, ws, (hipStream_t)stream);
}

// Y (M, N) bf16 = the posterior-weighted combination of every output row's three product rows (qd_gemm_fwd_mix).
QD_API int qd_gemm_fwd_skinny_mix(const uint16_t* A, const uint16_t* W, const uint16_t* bias, const float* P,
                                  uint16_t* Y, int M, int N, int K, int E, void* ws, void* stream) {
  if (E != 3 || !P) return (int)hipErrorInvalidValue;
  Args a{reinterpret_cast<const uint8_t*>(A), reinterpret_cast<const uint8_t*>(W), bias, nullptr, P, nullptr, nullptr,
         Y, nullptr, nullptr, M, N, K, E, 0};
  return qd::skinny::launch<false, true>(a, ws, (hipStream_t)stream);
}

// The e4m3 forms with per-row (rs) and per-channel (cs) power-of-two scales (qd_gemm_fwd_rows_f8 /
// qd_gemm_fwd_mix_rows_f8).
QD_API int qd_gemm_fwd_skinny_rows_f8(const uint8_t* A8, const uint8_t* W8, const float* rs, const float* cs,
                                      const uint16_t* bias, uint16_t* Y, int M, int N, int K, const long* expert, int E,
                                      void* ws, void* stream) {
  if (E < 1 || E > 64 || (expert == nullptr && E != 1) || !rs || !cs) return (int)hipErrorInvalidValue;
  Args a{A8, W8, bias, expert, nullptr, rs, cs, Y, nullptr, nullptr, M, N, K, E, 0};
  return qd::skinny::launch<true, false>(a, ws, (hipStream_t)stream);
}

QD_API int qd_gemm_fwd_skinny_mix_rows_f8(const uint8_t* A8, const uint8_t* W8, const float* rs, const float* cs,
                                          const uint16_t* bias, const float* P, uint16_t* Y, int M, int N, int K, int E,
                                          void* ws, void* stream) {
  if (E != 3 || !P || !rs || !cs) return (int)hipErrorInvalidValue;
  Args a{A8, W8, bias, nullptr, P, rs, cs, Y, nullptr, nullptr, M, N, K, E, 0};
  return qd::skinny::launch<true, true>(a, ws, (hipStream_t)stream);
}
