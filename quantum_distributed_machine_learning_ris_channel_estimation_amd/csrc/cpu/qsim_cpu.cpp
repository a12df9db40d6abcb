// CPU state-vector simulator (C++17 + OpenMP) for the QSC variational circuit.
//
// Same circuit as csrc/hip/qsim.hip (reference: Estimators_QuantumNAT_onchipQNN.py:125-142)
// but implemented independently and literally, gate by gate, in double precision:
// it is (a) the compute path of the CPU configuration ("4-qubit VQC, CPU state-vector
// sim, batch=32") and (b) the oracle the HIP kernels are tested against.
//
// Wire i <-> bit i of the basis index.  Backward is adjoint differentiation over the
// explicit gate list; per-sample weight gradients are summed in sample order so the
// result is deterministic for any thread count.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <vector>

#define QD_API extern "C" __attribute__((visibility("default")))

namespace {

using cd = std::complex<double>;

enum GateType { kRY = 0, kRZ = 1, kCNOT = 2 };

struct Gate {
  int type;
  int q;      // target wire
  int c;      // control wire (CNOT)
  int wparam; // index into flattened weights, -1 if none
  int xparam; // index into the sample's input angles, -1 if none
  double angle;
};

std::vector<Gate> build_circuit(const float* xs, const float* w, int n, int L) {
  std::vector<Gate> g;
  g.reserve(n + L * 3 * n);
  for (int i = 0; i < n; ++i) g.push_back({kRY, i, -1, -1, i, (double)xs[i]});
  for (int l = 0; l < L; ++l) {
    for (int i = 0; i < n; ++i) {
      const int p = (l * n + i) * 2;
      g.push_back({kRY, i, -1, p, -1, (double)w[p]});
      g.push_back({kRZ, i, -1, p + 1, -1, (double)w[p + 1]});
    }
    for (int i = 0; i + 1 < n; ++i) g.push_back({kCNOT, i + 1, i, -1, -1, 0.0});
    g.push_back({kCNOT, 0, n - 1, -1, -1, 0.0});
  }
  return g;
}

// Apply gate (or its adjoint) in place.
void apply(std::vector<cd>& s, const Gate& g, bool adjoint) {
  const size_t D = s.size();
  const size_t m = size_t(1) << g.q;
  if (g.type == kCNOT) {
    const size_t cm = size_t(1) << g.c;
    for (size_t k = 0; k < D; ++k)
      if ((k & cm) && !(k & m)) std::swap(s[k], s[k | m]);
    return;
  }
  const double a = adjoint ? -g.angle : g.angle;
  if (g.type == kRY) {
    const double c = std::cos(a / 2), sn = std::sin(a / 2);
    for (size_t k = 0; k < D; ++k) {
      if (k & m) continue;
      const cd a0 = s[k], a1 = s[k | m];
      s[k] = c * a0 - sn * a1;
      s[k | m] = sn * a0 + c * a1;
    }
  } else {  // RZ
    const cd e0 = std::polar(1.0, -a / 2), e1 = std::polar(1.0, a / 2);
    for (size_t k = 0; k < D; ++k) s[k] *= (k & m) ? e1 : e0;
  }
}

// Im <lam| G_gen |psi> where G_gen = Y (RY) or Z (RZ) on wire q.
double gen_im(const std::vector<cd>& lam, const std::vector<cd>& psi, const Gate& g) {
  const size_t D = psi.size();
  const size_t m = size_t(1) << g.q;
  cd acc = 0;
  if (g.type == kRZ) {
    for (size_t k = 0; k < D; ++k) acc += std::conj(lam[k]) * ((k & m) ? -psi[k] : psi[k]);
  } else {  // Y: (Y psi)_k = -i psi_{k^m} if bit 0, +i psi_{k^m} if bit 1
    const cd I(0, 1);
    for (size_t k = 0; k < D; ++k) acc += std::conj(lam[k]) * ((k & m) ? I : -I) * psi[k ^ m];
  }
  return acc.imag();
}

void forward_state(std::vector<cd>& s, const std::vector<Gate>& gates) {
  std::fill(s.begin(), s.end(), cd(0));
  s[0] = 1.0;
  for (const Gate& g : gates) apply(s, g, false);
}

}  // namespace

QD_API int qd_cpu_qsim_fwd(const float* x, const float* w, float* E, int B, int n, int L) {
  if (n < 1 || n > 24) return 1;
  const size_t D = size_t(1) << n;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<cd> s(D);
    forward_state(s, build_circuit(x + (size_t)b * n, w, n, L));
    for (int q = 0; q < n; ++q) {
      double e = 0;
      for (size_t k = 0; k < D; ++k) e += std::norm(s[k]) * (((k >> q) & 1) ? -1.0 : 1.0);
      E[(size_t)b * n + q] = (float)e;
    }
  }
  return 0;
}

QD_API int qd_cpu_qsim_bwd(const float* x, const float* w, const float* gE, float* dx, float* dw, int B, int n,
                           int L) {
  if (n < 1 || n > 24) return 1;
  const size_t D = size_t(1) << n;
  const int P = 2 * n * L;
  std::vector<double> per(size_t(B) * P, 0.0);
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    const auto gates = build_circuit(x + (size_t)b * n, w, n, L);
    std::vector<cd> psi(D), lam(D);
    forward_state(psi, gates);
    for (size_t k = 0; k < D; ++k) {
      double o = 0;
      for (int q = 0; q < n; ++q) o += (((k >> q) & 1) ? -1.0 : 1.0) * gE[(size_t)b * n + q];
      lam[k] = o * psi[k];
    }
    double* pw = per.data() + (size_t)b * P;
    for (int q = 0; q < n; ++q) dx[(size_t)b * n + q] = 0.f;
    for (int gi = (int)gates.size() - 1; gi >= 0; --gi) {
      const Gate& g = gates[gi];
      if (g.type != kCNOT) {
        const double d = gen_im(lam, psi, g);  // dL/dangle = 2 Re<lam| dG |psi_before> = Im<lam|Gen|psi_after>
        if (g.wparam >= 0) pw[g.wparam] += d;
        if (g.xparam >= 0) dx[(size_t)b * n + g.xparam] += (float)d;
      }
      apply(psi, g, true);
      apply(lam, g, true);
    }
  }
  for (int p = 0; p < P; ++p) {
    double t = 0;
    for (int b = 0; b < B; ++b) t += per[(size_t)b * P + p];
    dw[p] = (float)t;
  }
  return 0;
}

// ------------------------------------------------------------------------------- finite shots
// probs (B, 2^n) double = |amp_k|^2 of the final state, natural basis order (the oracle of qd_qsim_probs).
QD_API int qd_cpu_qsim_probs(const float* x, const float* w, double* probs, int B, int n, int L) {
  if (n < 1 || n > 24) return 1;
  const size_t D = size_t(1) << n;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<cd> s(D);
    forward_state(s, build_circuit(x + (size_t)b * n, w, n, L));
    for (size_t k = 0; k < D; ++k) probs[(size_t)b * D + k] = std::norm(s[k]);
  }
  return 0;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).
QD_API void qd_cpu_philox4x32(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4) {
  uint32_t c0 = ctr4[0], c1 = ctr4[1], c2 = ctr4[2], c3 = ctr4[3], k0 = key2[0], k1 = key2[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out4[0] = c0;
  out4[1] = c1;
  out4[2] = c2;
  out4[3] = c3;
}

// Finite-shot <Z_i> from fp32 probabilities, sequentially: the sampling contract of csrc/hip/qsim_shots.hip (see its
// header), bit for bit.  probs (B, 2^n) fp32, a normalised distribution; E (B, n) fp32; counts (B, n) int32, nullable.
namespace {
int sample_z_rows(const float* probs, float* E, int32_t* counts, int B, int n, int shots, uint64_t seed, uint64_t ctr,
                  int nmax) {
  if (n < 2 || n > nmax || shots < 1 || shots > (1 << 20)) return 1;
  const size_t D = size_t(1) << n;
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<uint32_t> cum(D);
    uint32_t run = 0;
    for (size_t k = 0; k < D; ++k) {
      const float p = probs[(size_t)b * D + k];
      run += p > 0.f ? (uint32_t)std::nearbyintf(p * 1073741824.f) : 0u;   // (default rounding mode: to nearest even)
      cum[k] = run;
    }
    const uint32_t T = run;
    std::vector<int32_t> c1(n, 0);
    uint32_t rnd[4] = {0, 0, 0, 0};
    for (int s = 0; s < shots; ++s) {
      if ((s & 3) == 0) {
        const uint32_t c4[4] = {(uint32_t)s >> 2, (uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32)};
        qd_cpu_philox4x32(c4, key, rnd);
      }
      const uint32_t t = (uint32_t)(((uint64_t)rnd[s & 3] * T) >> 32);
      // the smallest index with cum[k] > t (exists whenever T > 0; an all-zero row gives D - 1)
      size_t k = std::upper_bound(cum.begin(), cum.end(), t) - cum.begin();
      if (k > D - 1) k = D - 1;
      for (int i = 0; i < n; ++i) c1[i] += (int32_t)((k >> i) & 1);
    }
    for (int i = 0; i < n; ++i) {
      E[(size_t)b * n + i] = (float)(shots - 2 * c1[i]) / (float)shots;
      if (counts != nullptr) counts[(size_t)b * n + i] = c1[i];
    }
  }
  return 0;
}
}  // namespace

QD_API int qd_cpu_sample_z(const float* probs, float* E, int32_t* counts, int B, int n, int shots, uint64_t seed,
                           uint64_t ctr) {
  return sample_z_rows(probs, E, counts, B, n, shots, seed, ctr, 12);   // (the range of csrc/hip/qsim_shots.hip)
}

// The same contract for 2 <= n <= 16: the oracle of the streamed sampler (csrc/hip/qsim_stream_shots.hip) above 12.
QD_API int qd_cpu_sample_z_wide(const float* probs, float* E, int32_t* counts, int B, int n, int shots, uint64_t seed,
                                uint64_t ctr) {
  return sample_z_rows(probs, E, counts, B, n, shots, seed, ctr, 16);
}

// ------------------------------------------------------------------------------- Pauli noise (csrc/hip/qsim_noise.hip)
// The noise contract of csrc/hip/qsim_noise.hip (see its header), sequentially.
namespace {
inline uint32_t pauli_x(uint32_t p) { return ((p + 1u) >> 1) & 1u; }   // 0 .. 3 = I, X, Y, Z
inline uint32_t pauli_z(uint32_t p) { return (p >> 1) & 1u; }
inline bool noise_shape_ok(int n, int L) { return n >= 2 && n <= 12 && L >= 1 && 2 * n * L <= 4096; }
inline bool traj_ok(int shots, int T) {
  if (shots < 1 || shots > (1 << 20) || T < 1 || T > 1024 || shots % T != 0) return false;
  return T == 1 || (shots / T) % 4 == 0;
}
}  // namespace

// sites (B, T, L, n, 2) uint8: the error code drawn at every site (0: none; k = 0: 1 .. 3, k = 1: 1 .. 15).
// thr1 / thr2 (n) uint32 thresholds.
QD_API int qd_cpu_noise_sites(uint8_t* sites, const uint32_t* thr1, const uint32_t* thr2, int B, int n, int L, int T,
                              uint64_t seed, uint64_t ctr) {
  if (!noise_shape_ok(n, L) || B < 0 || T < 1 || T > 1024) return 1;
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int nsites = 2 * n * L;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    for (int tau = 0; tau < T; ++tau) {
      uint8_t* out = sites + ((size_t)b * T + tau) * nsites;
      uint32_t rnd[4] = {0, 0, 0, 0};
      for (int s = 0; s < nsites; ++s) {
        if ((s & 3) == 0) {
          const uint32_t c4[4] = {0x80000000u | ((uint32_t)tau << 10) | ((uint32_t)s >> 2), (uint32_t)b, (uint32_t)ctr,
                                  (uint32_t)(ctr >> 32)};
          qd_cpu_philox4x32(c4, key, rnd);
        }
        const int q = (s >> 1) % n, k = s & 1;
        const uint32_t r = rnd[s & 3], thr = k ? thr2[q] : thr1[q];
        out[s] = r < thr ? (uint8_t)(1u + (uint32_t)(((uint64_t)r * (k ? 15u : 3u)) / thr)) : (uint8_t)0;
      }
    }
  }
  return 0;
}

// frames (rows, L, 2) int32 = every layer's (a, b) from the site codes (rows, L, n, 2) uint8.
QD_API int qd_cpu_pauli_frames(const uint8_t* sites, int32_t* frames, int rows, int n, int L) {
  if (!noise_shape_ok(n, L) || rows < 0) return 1;
  for (size_t i = 0; i < (size_t)rows * L * n; ++i)
    if (sites[2 * i] > 3 || sites[2 * i + 1] > 15) return 1;
#pragma omp parallel for schedule(static)
  for (int r = 0; r < rows; ++r) {
    for (int l = 0; l < L; ++l) {
      const uint8_t* c = sites + ((size_t)r * L + l) * n * 2;
      uint32_t a = 0, z = 0;
      for (int q = 0; q < n; ++q) {
        a |= pauli_x(c[2 * q]) << q;
        z |= pauli_z(c[2 * q]) << q;
      }
      for (int q = 0; q < n; ++q) {
        const int t = (q + 1) % n;
        a ^= ((a >> q) & 1u) << t;
        z ^= ((z >> t) & 1u) << q;
        const uint32_t pc = c[2 * q + 1] >> 2, pt = c[2 * q + 1] & 3u;
        a ^= (pauli_x(pc) << q) ^ (pauli_x(pt) << t);
        z ^= (pauli_z(pc) << q) ^ (pauli_z(pt) << t);
      }
      frames[((size_t)r * L + l) * 2] = (int32_t)a;
      frames[((size_t)r * L + l) * 2 + 1] = (int32_t)z;
    }
  }
  return 0;
}

// probs (B, 2^n) double of the circuit with row b's frames (B, L, 2) int32 applied behind the rings of layers
// 0 .. L-2: A'[j] = (-1)^popc(b & (j ^ a)) A[j ^ a].  The last layer's frame is left out (it acts on the outcome).
QD_API int qd_cpu_qsim_probs_framed(const float* x, const float* w, const int32_t* frames, double* probs, int B, int n,
                                    int L) {
  if (!noise_shape_ok(n, L) || B < 0) return 1;
  const size_t D = size_t(1) << n;
  for (size_t i = 0; i < (size_t)B * L * 2; ++i)
    if (frames[i] < 0 || (size_t)frames[i] >= D) return 1;
  const int per = 3 * n;   // gates of a layer
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    const auto gates = build_circuit(x + (size_t)b * n, w, n, L);
    std::vector<cd> s(D, cd(0)), t(D);
    s[0] = 1.0;
    size_t gi = 0;
    for (; gi < (size_t)n; ++gi) apply(s, gates[gi], false);   // the embedding
    for (int l = 0; l < L; ++l) {
      for (int k = 0; k < per; ++k, ++gi) apply(s, gates[gi], false);
      if (l == L - 1) break;
      const size_t fa = (size_t)frames[((size_t)b * L + l) * 2], fb = (size_t)frames[((size_t)b * L + l) * 2 + 1];
      if (fa == 0 && fb == 0) continue;
      for (size_t j = 0; j < D; ++j) {
        const size_t js = j ^ fa;
        t[j] = (__builtin_popcountll(fb & js) & 1) ? -s[js] : s[js];
      }
      s.swap(t);
    }
    for (size_t k = 0; k < D; ++k) probs[(size_t)b * D + k] = std::norm(s[k]);
  }
  return 0;
}

// Noisy finite-shot <Z_i>: probs (B, T, 2^n) fp32, one distribution per trajectory; amask (B, T) int32, the last
// layer's X masks; thr_ro (n, 2) uint32 readout thresholds ([i][0]: reads 1 given 0, [i][1]: reads 0 given 1).
QD_API int qd_cpu_sample_z_noisy(const float* probs, const int32_t* amask, const uint32_t* thr_ro, float* E,
                                 int32_t* counts, int B, int n, int shots, int T, uint64_t seed, uint64_t ctr) {
  if (n < 2 || n > 12 || !traj_ok(shots, T) || B < 0) return 1;
  const size_t D = size_t(1) << n;
  for (size_t i = 0; i < (size_t)B * T; ++i)
    if (amask[i] < 0 || (size_t)amask[i] >= D) return 1;
  bool readout = false;
  for (int i = 0; i < 2 * n; ++i) {
    if (thr_ro[i] > 65535u) return 1;
    readout |= thr_ro[i] != 0;
  }
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int S = shots / T;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<uint32_t> cum(D);
    std::vector<int32_t> c1(n, 0);
    uint32_t rnd[4] = {0, 0, 0, 0}, ro[4] = {0, 0, 0, 0};
    uint32_t T_cdf = 0;
    for (int s = 0; s < shots; ++s) {
      const int tau = s / S;
      if (s % S == 0) {   // the trajectory's CDF
        uint32_t run = 0;
        const float* p = probs + ((size_t)b * T + tau) * D;
        for (size_t k = 0; k < D; ++k) {
          run += p[k] > 0.f ? (uint32_t)std::nearbyintf(p[k] * 1073741824.f) : 0u;
          cum[k] = run;
        }
        T_cdf = run;
      }
      if ((s & 3) == 0) {
        const uint32_t c4[4] = {(uint32_t)s >> 2, (uint32_t)b, (uint32_t)ctr, (uint32_t)(ctr >> 32)};
        qd_cpu_philox4x32(c4, key, rnd);
      }
      const uint32_t t = (uint32_t)(((uint64_t)rnd[s & 3] * T_cdf) >> 32);
      size_t k = std::upper_bound(cum.begin(), cum.end(), t) - cum.begin();
      if (k > D - 1) k = D - 1;
      k ^= (size_t)amask[(size_t)b * T + tau];
      if (readout) {
        for (int i = 0; i < n; ++i) {
          if ((i & 7) == 0) {
            const uint32_t c4[4] = {0x40000000u | ((uint32_t)s << 1) | ((uint32_t)i >> 3), (uint32_t)b, (uint32_t)ctr,
                                    (uint32_t)(ctr >> 32)};
            qd_cpu_philox4x32(c4, key, ro);
          }
          const uint32_t field = (ro[(i & 7) >> 1] >> (16 * (i & 1))) & 0xFFFFu;
          const uint32_t bit = (uint32_t)(k >> i) & 1u;
          if (field < thr_ro[2 * i + bit]) k ^= size_t(1) << i;
        }
      }
      for (int i = 0; i < n; ++i) c1[i] += (int32_t)((k >> i) & 1);
    }
    for (int i = 0; i < n; ++i) {
      E[(size_t)b * n + i] = (float)(shots - 2 * c1[i]) / (float)shots;
      if (counts != nullptr) counts[(size_t)b * n + i] = c1[i];
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------- exact noisy expectation
// The oracle of csrc/hip/qsim_mixed.hip (its header states the definition): the density matrix of the circuit under
// the Pauli channel qsim_noise.hip samples, taken in expectation, gate by gate in complex128.  rho[r, c] is entry
// r | c << n of a 2n-bit vector: a gate is U on bit q and conj(U) on bit n + q, so the state-vector `apply` runs it.
namespace {
// out += coef P rho P for the Pauli string with X mask xm and Z mask zm (Y = both): entry (r, c) takes
// (-1)^(popc(zm & r) + popc(zm & c)) rho[r ^ xm, c ^ xm] (the phases i, -i of the two sides cancel).
void pauli_conj_add(const std::vector<cd>& rho, std::vector<cd>& out, double coef, size_t xm, size_t zm, int n) {
  const size_t D = size_t(1) << n;
  for (size_t c = 0; c < D; ++c)
    for (size_t r = 0; r < D; ++r) {
      const bool neg = (__builtin_popcountll(zm & r) + __builtin_popcountll(zm & c)) & 1;
      const cd v = rho[(r ^ xm) | ((c ^ xm) << n)];
      out[r | (c << n)] += neg ? -coef * v : coef * v;
    }
}

// rho <- (1 - p) rho + (p / (4^k - 1)) sum over the non-identity Paulis on `wires` (k = 1 or 2 of them).
void pauli_channel(std::vector<cd>& rho, std::vector<cd>& tmp, double p, const int* wires, int k, int n) {
  if (p == 0.0) return;
  const int codes = 1 << (2 * k);
  for (size_t i = 0; i < rho.size(); ++i) tmp[i] = (1.0 - p) * rho[i];
  for (int code = 1; code < codes; ++code) {
    size_t xm = 0, zm = 0;
    for (int j = 0; j < k; ++j) {   // (code = 4 P_control + P_target: the first wire takes the high digit)
      const uint32_t pj = (uint32_t)(code >> (2 * (k - 1 - j))) & 3u;
      xm |= (size_t)pauli_x(pj) << wires[j];
      zm |= (size_t)pauli_z(pj) << wires[j];
    }
    pauli_conj_add(rho, tmp, p / (codes - 1), xm, zm, n);
  }
  rho.swap(tmp);
}

void apply_rho(std::vector<cd>& rho, int type, int q, int c, double angle, int n) {
  apply(rho, Gate{type, q, c, -1, -1, angle}, false);
  apply(rho, Gate{type, q + n, c < 0 ? -1 : c + n, -1, -1, type == kRZ ? -angle : angle}, false);
}
}  // namespace

// probs (B, 2^n) double: the diagonal of rho behind the last ring, natural basis order, before the readout.
// thr1 / thr2 (n) uint32: the gate thresholds, p = thr / 2^32.  2 <= n <= 8, L >= 1, 2 n L <= 4096.
QD_API int qd_cpu_qsim_mixed_probs(const float* x, const float* w, const uint32_t* thr1, const uint32_t* thr2,
                                   double* probs, int B, int n, int L) {
  if (n < 2 || n > 8 || L < 1 || 2 * n * L > 4096 || B < 0) return 1;
  const size_t D = size_t(1) << n;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<cd> rho(D * D, cd(0)), tmp(D * D);
    rho[0] = 1.0;
    for (int l = 0; l < L; ++l) {
      for (int q = 0; q < n; ++q) {
        const int p = (l * n + q) * 2;
        if (l == 0) apply_rho(rho, kRY, q, -1, (double)x[(size_t)b * n + q], n);
        apply_rho(rho, kRY, q, -1, (double)w[p], n);
        apply_rho(rho, kRZ, q, -1, (double)w[p + 1], n);
        pauli_channel(rho, tmp, (double)thr1[q] / 4294967296.0, &q, 1, n);
      }
      for (int q = 0; q < n; ++q) {
        const int wires[2] = {q, (q + 1) % n};
        apply_rho(rho, kCNOT, wires[1], wires[0], 0.0, n);
        pauli_channel(rho, tmp, (double)thr2[q] / 4294967296.0, wires, 2, n);
      }
    }
    for (size_t k = 0; k < D; ++k) probs[(size_t)b * D + k] = rho[k | (k << n)].real();
  }
  return 0;
}

// The host twin of qd_qsim_mixed_adjoint (csrc/hip/qsim_mixed.hip states the method), in complex128 and in the
// oracle's gate order reversed.  Lam[r, c] is stored like rho; <Lam, rho> = Re sum conj(Lam) rho.
namespace {
// A <- a A + k I (x) tr_wires A on the k wires (1 or 2): the site's map D, or with (1 / a, -k / a) its inverse.
void site_map(std::vector<cd>& A, double a, double k, const int* wires, int nw, int n) {
  size_t rm = 0;
  for (int j = 0; j < nw; ++j) rm |= size_t(1) << wires[j];
  const size_t both = rm | (rm << n);
  for (size_t base = 0; base < A.size(); ++base) {
    if (base & both) continue;
    cd s = 0;
    for (size_t v = rm;; v = (v - 1) & rm) {   // the block's diagonal: equal row and column bits on the wires
      s += A[base | v | (v << n)];
      if (v == 0) break;
    }
    for (size_t r = rm;; r = (r - 1) & rm) {
      for (size_t c = rm;; c = (c - 1) & rm) {
        cd& e = A[base | r | (c << n)];
        e = r == c ? a * e + k * s : a * e;
        if (c == 0) break;
      }
      if (r == 0) break;
    }
  }
}

// <Lam, (-i/2) [P_q, rho]> for P = Z (type kRZ) or Y (kRY): the derivative by the rotation's angle.
double generator_term(const std::vector<cd>& lam, const std::vector<cd>& rho, int type, int q, int n) {
  const size_t m0 = size_t(1) << q, m1 = size_t(1) << (n + q);
  double acc = 0;
  for (size_t base = 0; base < rho.size(); ++base) {
    if (base & (m0 | m1)) continue;
    const cd p0 = rho[base], p1 = rho[base | m0], p2 = rho[base | m1], p3 = rho[base | m0 | m1];
    const cd l0 = lam[base], l1 = lam[base | m0], l2 = lam[base | m1], l3 = lam[base | m0 | m1];
    if (type == kRZ)
      acc += (std::conj(l1) * cd(0, 1) * p1 + std::conj(l2) * cd(0, -1) * p2).real();
    else
      acc += 0.5 * (std::conj(l1 + l2) * (p0 - p3) - std::conj(l0 - l3) * (p1 + p2)).real();
  }
  return acc;
}
}  // namespace

// G (B, 2 n L) double: row b the gradient of sum_j gE[b, j] E[b, j], column (l n + q) 2 + k for w[l, q, k].
// E (nullable; B, n) double: the expectation with the readout.  thr_ro (n, 2).  The ranges of
// qd_cpu_qsim_mixed_probs; a gate threshold above 2^31 (p > 1/2) is refused.  Nothing is written on a refusal.
QD_API int qd_cpu_qsim_mixed_adjoint(const float* x, const float* w, const uint32_t* thr1, const uint32_t* thr2,
                                     const uint32_t* thr_ro, const float* gE, double* G, double* E, int B, int n,
                                     int L) {
  if (n < 2 || n > 8 || L < 1 || 2 * n * L > 4096 || B < 0) return 1;
  if (!x || !w || !thr1 || !thr2 || !thr_ro || !gE || !G) return 1;
  for (int q = 0; q < n; ++q)
    if (thr1[q] > 0x80000000u || thr2[q] > 0x80000000u) return 1;
  const size_t D = size_t(1) << n;
  const int P = 2 * n * L;
#pragma omp parallel for schedule(static)
  for (int b = 0; b < B; ++b) {
    std::vector<cd> rho(D * D, cd(0)), lam(D * D, cd(0)), tmp(D * D);
    rho[0] = 1.0;
    const float* xs = x + (size_t)b * n;
    for (int l = 0; l < L; ++l) {
      for (int q = 0; q < n; ++q) {
        const int p = (l * n + q) * 2;
        if (l == 0) apply_rho(rho, kRY, q, -1, (double)xs[q], n);
        apply_rho(rho, kRY, q, -1, (double)w[p], n);
        apply_rho(rho, kRZ, q, -1, (double)w[p + 1], n);
        pauli_channel(rho, tmp, (double)thr1[q] / 4294967296.0, &q, 1, n);
      }
      for (int q = 0; q < n; ++q) {
        const int wires[2] = {q, (q + 1) % n};
        apply_rho(rho, kCNOT, wires[1], wires[0], 0.0, n);
        pauli_channel(rho, tmp, (double)thr2[q] / 4294967296.0, wires, 2, n);
      }
    }
    std::vector<double> gc(n);
    for (int j = 0; j < n; ++j) {
      const double c = 1.0 - ((double)thr_ro[2 * j] + (double)thr_ro[2 * j + 1]) / 65536.0;
      gc[j] = (double)gE[(size_t)b * n + j] * c;
      if (E != nullptr) {
        double S = 0;
        for (size_t k = 0; k < D; ++k) S += ((k >> j) & 1) ? -rho[k | (k << n)].real() : rho[k | (k << n)].real();
        E[(size_t)b * n + j] = c * S + ((double)thr_ro[2 * j + 1] - (double)thr_ro[2 * j]) / 65536.0;
      }
    }
    for (size_t k = 0; k < D; ++k) {
      double v = 0;
      for (int j = 0; j < n; ++j) v += ((k >> j) & 1) ? -gc[j] : gc[j];
      lam[k | (k << n)] = v;
    }
    for (int l = L - 1; l >= 0; --l) {
      for (int q = n - 1; q >= 0; --q) {
        const int wires[2] = {q, (q + 1) % n};
        const double p2 = (double)thr2[q] / 4294967296.0, a = 1.0 - 16.0 * p2 / 15.0, k = 4.0 * p2 / 15.0;
        site_map(rho, 1.0 / a, -k / a, wires, 2, n);
        site_map(lam, a, k, wires, 2, n);
        apply_rho(rho, kCNOT, wires[1], wires[0], 0.0, n);
        apply_rho(lam, kCNOT, wires[1], wires[0], 0.0, n);
      }
      for (int q = n - 1; q >= 0; --q) {
        const int p = (l * n + q) * 2;
        const double p1 = (double)thr1[q] / 4294967296.0, a = 1.0 - 4.0 * p1 / 3.0, k = 2.0 * p1 / 3.0;
        const double theta = (double)w[p] + (l == 0 ? (double)xs[q] : 0.0), phi = (double)w[p + 1];
        site_map(rho, 1.0 / a, -k / a, &q, 1, n);
        site_map(lam, a, k, &q, 1, n);
        G[(size_t)b * P + p + 1] = generator_term(lam, rho, kRZ, q, n);
        apply_rho(rho, kRZ, q, -1, -phi, n);
        apply_rho(lam, kRZ, q, -1, -phi, n);
        G[(size_t)b * P + p] = generator_term(lam, rho, kRY, q, n);
        apply_rho(rho, kRY, q, -1, -theta, n);
        apply_rho(lam, kRY, q, -1, -theta, n);
      }
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------- QOC gradient pruning
// The host twin of qd_qoc_update (csrc/hip/qoc.hip; the contract is stated at the top of that file), sequentially:
// bit-identical acc, mask and step.
QD_API int qd_cpu_qoc_update(float* acc, uint8_t* mask, int64_t* step, const float* grad, int P, int wa, int wp, int K,
                             uint64_t seed) {
  if (!acc || !mask || !step || !grad || P < 2 || P > 4096 || wa < 1 || wa > (1 << 20) || wp < 1 || wp > (1 << 20) ||
      K < 1 || K > P)
    return 1;
  const uint64_t s = (uint64_t)*step, period = (uint64_t)(wa + wp), t = s % period, s1 = s + 1, t1 = s1 % period;
  if (t == 0)
    for (int p = 0; p < P; ++p) acc[p] = 0.f;
  if (t < (uint64_t)wa) {
    for (int p = 0; p < P; ++p) {
      const float g = std::fabs(grad[p]), a1 = acc[p] + g;
      if (std::isfinite(g) && std::isfinite(a1)) acc[p] = a1;
    }
  }
  if (t1 < (uint64_t)wa) {
    for (int p = 0; p < P; ++p) mask[p] = 1;
  } else {
    float m = 0.f;
    for (int p = 0; p < P; ++p) m = std::max(m, acc[p]);
    std::vector<uint32_t> q(P);
    uint64_t S = 0;
    for (int p = 0; p < P; ++p) {
      q[p] = m > 0.f ? (uint32_t)std::floor((acc[p] / m) * 1048576.f) + 1u : 1u;
      S += q[p];
      mask[p] = 0;
    }
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t rnd[4] = {0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
      if ((k & 3) == 0) {
        const uint32_t c4[4] = {0x20000000u | (uint32_t)(k >> 2), 0u, (uint32_t)s1, (uint32_t)(s1 >> 32)};
        qd_cpu_philox4x32(c4, key, rnd);
      }
      const uint64_t u = rnd[k & 3];
      const uint64_t r = u * (S >> 32) + ((u * (S & 0xFFFFFFFFull)) >> 32);
      uint64_t run = 0;
      for (int p = 0; p < P; ++p) {
        run += q[p];
        if (run > r) {   // (a chosen parameter's q is 0: it cannot be the first to exceed r)
          S -= q[p];
          q[p] = 0;
          mask[p] = 1;
          break;
        }
      }
    }
  }
  *step = (int64_t)s1;
  return 0;
}
