// QuantumNAT post-measurement normalization and quantization fused into the QSC heads (ops/postmeas.py is the
// definition these kernels are held to; csrc/hip/qsc.hip has the plain heads they replace when the model has a
// PostMeasurement module).
//
//   mu_j = mean_b E[b, j]     v_j = mean_b (E[b, j] - mu_j)^2  (two passes)     z = (E - mu) rsqrt(v + eps)
//   K >= 2:  D = 2 R / (K - 1),  Q(z) = -R + D rint((clamp(z, -R, R) + R) / D)  (ties to even),  y = Q(z);  else y = z
//   logits = Wc y + bc -> log_softmax -> mean NLL;   loss = NLL + qweight * sum (z - Q)^2 / (B n)
//   g = dloss/dz = [|z| <= R] dNLL/dy + 2 qweight (z - Q) / (B n)            (straight-through, Q constant)
//   dE = rsqrt(v + eps) (g - mean_b g - z mean_b (g z))                      (through the batch statistics)
//
// Training head: ONE workgroup of 1024 threads, like qsc_head_kernel; thread t owns rows t, t + 1024, ...  Every
// reduction is: the thread's rows in ascending order, a wave butterfly, the 16 wave partials summed in wave order by
// one thread -- a fixed order, no float atomics, so every output is bit-identical run to run.  g makes its round trip
// through dE (each thread re-reads only what it wrote itself).
#include "common.h"

namespace qd {
namespace qsc {

constexpr int PM_NT = 1024, PM_NW = PM_NT / 64;

// rows a thread keeps in registers across the phases (the step's 2304 rows are three per thread); wider heads
// re-read E instead: their gradient accumulators already fill the 128 VGPRs a 1024-thread workgroup leaves a wave
template <int N>
struct PmKeep {
  static constexpr int value = N <= 8 ? 3 : 0;
};

__device__ __forceinline__ float pm_quant(float z, float R, float inv_d, float d) {
  const float zc = fminf(fmaxf(z, -R), R);
  return -R + d * rintf((zc + R) * inv_d);
}

// Column sums of the NV per-thread values v[] over the workgroup: fin[k] = sum over waves (in order) of the wave sums.
template <int NV>
__device__ __forceinline__ void pm_block_sums(const float (&v)[NV], float (*red)[NV], float* fin) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float s = wave_sum(v[k]);
    if (lane == 0) red[wv][k] = s;
  }
  __syncthreads();
  if (t < NV) {
    float s = 0.f;
    for (int w = 0; w < PM_NW; ++w) s += red[w][t];
    fin[t] = s;
  }
  __syncthreads();
}

template <int N, int C>
__global__ void __launch_bounds__(PM_NT) qsc_head_pm_kernel(
    const float* __restrict__ E, const float* __restrict__ wc, const float* __restrict__ bc,
    const long* __restrict__ labels, float* __restrict__ dE, float* __restrict__ dwc, float* __restrict__ dbc,
    float* __restrict__ loss, float* __restrict__ loss_acc, float* __restrict__ skip, int skip_add, int accumulate,
    int B, float* __restrict__ run_mean, float* __restrict__ run_var, float momentum, float eps, int levels,
    float qrange, float qweight, float* __restrict__ z_out) {
  constexpr int P = C * N + C;
  constexpr int TOT = P + 2;           // head grads | NLL sum | penalty sum
  constexpr int KEEP = PmKeep<N>::value;
  __shared__ float red[PM_NW][TOT];
  __shared__ float redn[PM_NW][N];
  __shared__ float red2[PM_NW][2 * N];
  __shared__ float fin[TOT], fin2[2 * N];   // fin2: sum g | sum g z
  __shared__ float s_mu[N], s_var[N], s_rstd[N];
  const int t = threadIdx.x;
  const float invB = 1.f / (float)B;
  const bool quant = levels >= 2;
  const float R = qrange, d = quant ? 2.f * qrange / (float)(levels - 1) : 1.f, inv_d = 1.f / d;
  const float pw = quant ? qweight * invB / (float)N : 0.f;   // the penalty's weight per element

  float ek[KEEP > 0 ? KEEP : 1][N];
#pragma unroll
  for (int k = 0; k < KEEP; ++k) {
    const int b = t + k * PM_NT;
#pragma unroll
    for (int j = 0; j < N; ++j) ek[k][j] = b < B ? E[(size_t)b * N + j] : 0.f;
  }
  // f(e, b) for every row b of this thread, ascending: the kept rows from registers, the others from E
  auto rows = [&](auto&& f) {
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const int b = t + k * PM_NT;
      if (b < B) f(ek[k], b);
    }
    for (int b = t + KEEP * PM_NT; b < B; b += PM_NT) {
      float e[N];
#pragma unroll
      for (int j = 0; j < N; ++j) e[j] = E[(size_t)b * N + j];
      f(e, b);
    }
  };

  // phase 1: per-wire mean
  {
    float s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.f;
    rows([&](const float (&e)[N], int) {
#pragma unroll
      for (int j = 0; j < N; ++j) s[j] += e[j];
    });
    pm_block_sums<N>(s, redn, s_mu);
    if (t < N) s_mu[t] *= invB;
    __syncthreads();
  }
  // phase 2: per-wire variance about that mean (E[x^2] - mu^2 cancels when noise has squeezed a wire's spread)
  {
    float s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.f;
    rows([&](const float (&e)[N], int) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float c = e[j] - s_mu[j];
        s[j] += c * c;
      }
    });
    pm_block_sums<N>(s, redn, s_var);
    if (t < N) {
      const float v = s_var[t] * invB;
      s_var[t] = v;
      s_rstd[t] = 1.f / sqrtf(v + eps);
    }
    __syncthreads();
  }
  // phase 3: normalize, quantize, head forward + backward to g = dloss/dz (parked in dE)
  float acc[TOT];
#pragma unroll
  for (int k = 0; k < TOT; ++k) acc[k] = 0.f;
  rows([&](const float (&e)[N], int b) {
    float z[N], y[N], lg[C];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      z[j] = (e[j] - s_mu[j]) * s_rstd[j];
      y[j] = quant ? pm_quant(z[j], R, inv_d, d) : z[j];
    }
    if (z_out) {
#pragma unroll
      for (int j = 0; j < N; ++j) z_out[(size_t)b * N + j] = z[j];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float s = bc[c];
#pragma unroll
      for (int j = 0; j < N; ++j) s += wc[c * N + j] * y[j];
      lg[c] = s;
      mx = fmaxf(mx, s);
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
    const float lse = mx + __logf(se);
    const int lab = (int)labels[b];
    float ly = 0.f, dy[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dy[j] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ly += (c == lab) ? lg[c] : 0.f;
      const float gl = (__expf(lg[c] - lse) - (c == lab ? 1.f : 0.f)) * invB;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        dy[j] += gl * wc[c * N + j];
        acc[c * N + j] += gl * y[j];
      }
      acc[C * N + c] += gl;
    }
    acc[P] += lse - ly;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float g = dy[j];
      if (quant) {
        const float r = z[j] - y[j];
        acc[P + 1] += r * r;
        g = (fabsf(z[j]) <= R ? g : 0.f) + 2.f * pw * r;
      }
      dE[(size_t)b * N + j] = g;
    }
  });
  pm_block_sums<TOT>(acc, red, fin);
  // phase 4: per-wire sum g and sum g z (a pass of its own: 2 n more accumulators would not fit beside phase 3's)
  {
    float s[2 * N];
#pragma unroll
    for (int j = 0; j < 2 * N; ++j) s[j] = 0.f;
    rows([&](const float (&e)[N], int b) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float z = (e[j] - s_mu[j]) * s_rstd[j];
        const float g = dE[(size_t)b * N + j];
        s[j] += g;
        s[N + j] += g * z;
      }
    });
    pm_block_sums<2 * N>(s, red2, fin2);
  }
  const float nll = fin[P] * invB, total = nll + (quant ? qweight * fin[P + 1] * invB / (float)N : 0.f);
  if (t < C * N) dwc[t] = (accumulate ? dwc[t] : 0.f) + fin[t];
  else if (t < P) dbc[t - C * N] = (accumulate ? dbc[t - C * N] : 0.f) + fin[t];
  else if (t == P) {
    loss[0] = total;
    if (loss_acc) loss_acc[0] += total;
    if (skip) {  // NaN guard: a non-finite loss turns the optimizer step into a no-op
      const float bad = isfinite(total) ? 0.f : 1.f;
      skip[0] = skip_add ? skip[0] + bad : bad;
    }
  }
  // the running statistics, one thread per wire, now that the loss is known: a skipped step leaves them alone (a NaN
  // would sit in the buffers forever)
  if (t >= PM_NT - N && isfinite(total)) {
    const int j = t - (PM_NT - N);
    run_mean[j] = (1.f - momentum) * run_mean[j] + momentum * s_mu[j];
    run_var[j] = (1.f - momentum) * run_var[j] + momentum * (s_var[j] * ((float)B / (float)(B - 1)));
  }
  // phase 5: dE through the batch statistics
  rows([&](const float (&e)[N], int b) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float z = (e[j] - s_mu[j]) * s_rstd[j];
      const float g = dE[(size_t)b * N + j];
      dE[(size_t)b * N + j] = s_rstd[j] * (g - fin2[j] * invB - z * (fin2[N + j] * invB));
    }
  });
}

// Inference head with post-measurement processing: a thread per sample, like qsc_infer_head_kernel.  Batch mode takes
// the statistics over the first Bv rows; EVERY workgroup computes them itself, all in the same order (thread t of 256
// sums rows t, t + 256, ... ascending, a wave butterfly, the 4 wave partials in wave order), so all workgroups hold
// bit-identical statistics without a second launch or a grid hand-over: 4096 x 16 floats come from L2.
template <int N, int C>
__global__ void __launch_bounds__(256) qsc_infer_head_pm_kernel(
    const float* __restrict__ E, const float* __restrict__ wc, const float* __restrict__ bc, float* __restrict__ logp,
    long* __restrict__ pred, int B, int Bv, int running, const float* __restrict__ run_mean,
    const float* __restrict__ run_var, float eps, int levels, float qrange) {
  __shared__ float red[4][N];
  __shared__ float s_mu[N], s_rstd[N];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (running) {
    if (t < N) {
      s_mu[t] = run_mean[t];
      s_rstd[t] = 1.f / sqrtf(run_var[t] + eps);
    }
    __syncthreads();
  } else {
    const float invB = 1.f / (float)Bv;
    for (int pass = 0; pass < 2; ++pass) {
      float s[N];
#pragma unroll
      for (int j = 0; j < N; ++j) s[j] = 0.f;
      for (int b = t; b < Bv; b += 256) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float e = E[(size_t)b * N + j];
          const float c = pass ? e - s_mu[j] : e;
          s[j] += pass ? c * c : c;
        }
      }
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float v = wave_sum(s[j]);
        if (lane == 0) red[wv][j] = v;
      }
      __syncthreads();
      if (t < N) {
        const float v = (red[0][t] + red[1][t] + red[2][t] + red[3][t]) * invB;
        if (pass) s_rstd[t] = 1.f / sqrtf(v + eps);
        else s_mu[t] = v;
      }
      __syncthreads();
    }
  }
  const int b = blockIdx.x * 256 + t;
  if (b >= B) return;
  const bool quant = levels >= 2;
  const float d = quant ? 2.f * qrange / (float)(levels - 1) : 1.f, inv_d = 1.f / d;
  float y[N], lg[C], mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float z = (E[(size_t)b * N + j] - s_mu[j]) * s_rstd[j];
    y[j] = quant ? pm_quant(z, qrange, inv_d, d) : z;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float s = bc[c];
#pragma unroll
    for (int j = 0; j < N; ++j) s += wc[c * N + j] * y[j];
    lg[c] = s;
    mx = fmaxf(mx, s);
  }
  float se = 0.f;
  int am = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    se += __expf(lg[c] - mx);
    if (lg[c] > lg[am]) am = c;
  }
  const float lse = mx + __logf(se);
  if (logp) {
#pragma unroll
    for (int c = 0; c < C; ++c) logp[(size_t)b * C + c] = lg[c] - lse;
  }
  if (pred) pred[b] = am;
}

}  // namespace qsc
}  // namespace qd

using namespace qd::qsc;

// qd_qsc_head's arguments, then the PostMeasurement module's: running buffers (n,), momentum, eps, levels (0: no
// quantizer), qrange, the penalty's weight, and z_out (B, n; nullable): the normalized values.
QD_API int qd_qsc_head_pm(const float* E, const float* wc, const float* bc, const long* labels, float* dE, float* dwc,
                          float* dbc, float* loss, float* loss_acc, float* skip, int skip_add, int accumulate, int B,
                          int n, int C, float* run_mean, float* run_var, float momentum, float eps, int levels,
                          float qrange, float qweight, float* z_out, void* stream) {
  if (B < 2 || levels < 0 || levels == 1 || !(qrange > 0.f) || !run_mean || !run_var || !E || !dE)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
#define QD_HEADPM(NN, CC)                                                                                       \
  if (n == NN && C == CC) {                                                                                     \
    hipLaunchKernelGGL((qsc_head_pm_kernel<NN, CC>), dim3(1), dim3(PM_NT), 0, s, E, wc, bc, labels, dE, dwc, dbc, \
                       loss, loss_acc, skip, skip_add, accumulate, B, run_mean, run_var, momentum, eps, levels,  \
                       qrange, qweight, z_out);                                                                 \
    return (int)hipGetLastError();                                                                              \
  }
#define QD_HEADPM_N(NN) QD_HEADPM(NN, 2) QD_HEADPM(NN, 3) QD_HEADPM(NN, 4)
  QD_HEADPM_N(2) QD_HEADPM_N(3) QD_HEADPM_N(4) QD_HEADPM_N(5) QD_HEADPM_N(6) QD_HEADPM_N(7) QD_HEADPM_N(8)
  QD_HEADPM_N(9) QD_HEADPM_N(10) QD_HEADPM_N(11) QD_HEADPM_N(12) QD_HEADPM_N(13) QD_HEADPM_N(14) QD_HEADPM_N(15)
  QD_HEADPM_N(16)
#undef QD_HEADPM_N
#undef QD_HEADPM
  return (int)hipErrorInvalidValue;
}

// qd_qsc_infer_head's arguments, then: B_valid (the rows the batch statistics go over; the others are padding and
// still get an output), stats_mode (0: the batch's statistics, 1: the running ones), the running buffers, eps,
// levels, qrange.
QD_API int qd_qsc_infer_head_pm(const float* E, const float* wc, const float* bc, float* logp, long* pred, int B, int n,
                                int C, int B_valid, int stats_mode, const float* run_mean, const float* run_var,
                                float eps, int levels, float qrange, void* stream) {
  if (B < 1 || B_valid < 1 || B_valid > B || levels < 0 || levels == 1 || !(qrange > 0.f) || !E ||
      (stats_mode != 0 && stats_mode != 1) || (stats_mode == 1 && (!run_mean || !run_var)))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int grid = (B + 255) / 256;
#define QD_IHPM(NN, CC)                                                                                         \
  if (n == NN && C == CC) {                                                                                     \
    hipLaunchKernelGGL((qsc_infer_head_pm_kernel<NN, CC>), dim3(grid), dim3(256), 0, s, E, wc, bc, logp, pred, B, \
                       B_valid, stats_mode, run_mean, run_var, eps, levels, qrange);                            \
    return (int)hipGetLastError();                                                                              \
  }
#define QD_IHPM_N(NN) QD_IHPM(NN, 2) QD_IHPM(NN, 3) QD_IHPM(NN, 4)
  QD_IHPM_N(2) QD_IHPM_N(3) QD_IHPM_N(4) QD_IHPM_N(5) QD_IHPM_N(6) QD_IHPM_N(7) QD_IHPM_N(8) QD_IHPM_N(9)
  QD_IHPM_N(10) QD_IHPM_N(11) QD_IHPM_N(12) QD_IHPM_N(13) QD_IHPM_N(14) QD_IHPM_N(15) QD_IHPM_N(16)
#undef QD_IHPM_N
#undef QD_IHPM
  return (int)hipErrorInvalidValue;
}
