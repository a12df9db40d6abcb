// Host sanitizer driver for the density-matrix adjoint of the C++ CPU simulator (qd_cpu_qsim_mixed_adjoint).  Built
// with -fsanitize=address,undefined by tests/test_mixed_adjoint_cpu.py; links the simulator source directly, so no
// preload is needed.  Checks:
//   * at n = 2, 4, 6, with per-wire rates that include 0 and 0.5, every entry of G against the +-pi/2 shift rule over
//     qd_cpu_qsim_mixed_probs within 1e-5 sum|gE| (the rule is exact; the fp32 shifted angle moves it by 2^-22 sum|gE|);
//   * E equals the readout of those probabilities within 1e-12, and the same call repeats bit for bit;
//   * n = 8 runs (one sample, one layer) and gives finite rows;
//   * out-of-range arguments, null pointers and a rate above 0.5 are refused and leave the outputs untouched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int qd_cpu_qsim_mixed_probs(const float* x, const float* w, const uint32_t* thr1, const uint32_t* thr2,
                                       double* probs, int B, int n, int L);
extern "C" int qd_cpu_qsim_mixed_adjoint(const float* x, const float* w, const uint32_t* thr1, const uint32_t* thr2,
                                         const uint32_t* thr_ro, const float* gE, double* G, double* E, int B, int n,
                                         int L);

static int failures = 0;
static void expect(bool ok, const char* what, int n, int p) {
  if (!ok) {
    std::printf("FAILED %s (n=%d p=%d)\n", what, n, p);
    ++failures;
  }
}

// E (B, n) of the oracle's probabilities under the readout thresholds
static std::vector<double> readout(const std::vector<double>& probs, const std::vector<uint32_t>& thr_ro, int B, int n) {
  const int D = 1 << n;
  std::vector<double> E((size_t)B * n);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < n; ++j) {
      double S = 0;
      for (int k = 0; k < D; ++k) S += ((k >> j) & 1) ? -probs[(size_t)b * D + k] : probs[(size_t)b * D + k];
      const double c = 1.0 - ((double)thr_ro[2 * j] + (double)thr_ro[2 * j + 1]) / 65536.0;
      E[(size_t)b * n + j] = c * S + ((double)thr_ro[2 * j + 1] - (double)thr_ro[2 * j]) / 65536.0;
    }
  return E;
}

int main() {
  std::mt19937 rng(9876);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const int ns[] = {2, 4, 6, 8};
  for (int n : ns) {
    const int B = n == 8 ? 1 : 2, L = n == 8 ? 1 : 2, D = 1 << n, P = 2 * n * L;
    std::vector<float> x(B * n), w(P), gE(B * n);
    for (auto& v : x) v = U(rng);
    for (auto& v : w) v = 3.14159f * (1.f + U(rng));
    for (auto& v : gE) v = U(rng);
    std::vector<uint32_t> thr1(n), thr2(n), thr_ro(2 * n);
    for (int q = 0; q < n; ++q) {
      thr1[q] = (uint32_t)((0x80000000ull * q) / (n - 1));
      thr2[q] = (uint32_t)((0x80000000ull * (n - 1 - q)) / (n - 1));
      thr_ro[2 * q] = (uint32_t)(6000 * q / n);
      thr_ro[2 * q + 1] = (uint32_t)(30000 - 3000 * q);
    }
    std::vector<double> G((size_t)B * P, -7.0), G2((size_t)B * P, -7.0), E((size_t)B * n, -7.0);
    if (qd_cpu_qsim_mixed_adjoint(x.data(), w.data(), thr1.data(), thr2.data(), thr_ro.data(), gE.data(), G.data(),
                                  E.data(), B, n, L))
      return 2;
    if (qd_cpu_qsim_mixed_adjoint(x.data(), w.data(), thr1.data(), thr2.data(), thr_ro.data(), gE.data(), G2.data(),
                                  nullptr, B, n, L))
      return 2;
    for (size_t i = 0; i < G.size(); ++i) {
      expect(std::isfinite(G[i]), "finite", n, (int)i);
      expect(G[i] == G2[i], "repeatable, with and without E", n, (int)i);
    }
    std::vector<double> probs((size_t)B * D);
    if (qd_cpu_qsim_mixed_probs(x.data(), w.data(), thr1.data(), thr2.data(), probs.data(), B, n, L)) return 3;
    const std::vector<double> E0 = readout(probs, thr_ro, B, n);
    for (size_t i = 0; i < E.size(); ++i) expect(std::fabs(E[i] - E0[i]) <= 1e-12, "E is the oracle's", n, (int)i);
    if (n == 8) continue;   // (the shift rule's 4 n L forwards stay at the small sizes)
    for (int p = 0; p < P; ++p) {
      std::vector<double> Es[2];
      for (int s = 0; s < 2; ++s) {
        std::vector<float> ws(w);
        ws[p] += s == 0 ? 1.57079632679f : -1.57079632679f;
        if (qd_cpu_qsim_mixed_probs(x.data(), ws.data(), thr1.data(), thr2.data(), probs.data(), B, n, L)) return 3;
        Es[s] = readout(probs, thr_ro, B, n);
      }
      for (int b = 0; b < B; ++b) {
        double want = 0, scale = 0;
        for (int j = 0; j < n; ++j) {
          want += 0.5 * gE[b * n + j] * (Es[0][(size_t)b * n + j] - Es[1][(size_t)b * n + j]);
          scale += std::fabs(gE[b * n + j]);
        }
        expect(std::fabs(G[(size_t)b * P + p] - want) <= 1e-5 * scale, "the shift rule", n, p);
      }
    }
  }
  // refusals: nothing is written
  float e[8] = {0};
  uint32_t thr[16] = {0}, big[16] = {0};
  big[1] = 0x80000001u;
  double d[8];
  for (double& v : d) v = -7.0;
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, 1, 1, 1) != 0, "n = 1 refused", 1, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, 1, 9, 1) != 0, "n = 9 refused", 9, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, 1, 2, 0) != 0, "L = 0 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, 1, 2, 1025) != 0, "2 n L > 4096 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, -1, 2, 1) != 0, "B < 0 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, nullptr, d, d + 4, 1, 2, 1) != 0, "null gE refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, nullptr, d + 4, 1, 2, 1) != 0, "null G refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, big, thr, thr, e, d, d + 4, 1, 2, 1) != 0, "p1 > 0.5 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, big, thr, e, d, d + 4, 1, 2, 1) != 0, "p2 > 0.5 refused", 2, 0);
  for (double v : d) expect(v == -7.0, "a refused call writes nothing", 0, 0);
  expect(qd_cpu_qsim_mixed_adjoint(e, e, thr, thr, thr, e, d, d + 4, 1, 2, 1) == 0, "the admitted call runs", 2, 0);
  std::printf("qsim_mixed_adjoint_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
