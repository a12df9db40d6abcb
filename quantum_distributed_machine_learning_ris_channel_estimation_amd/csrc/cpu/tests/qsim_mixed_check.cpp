// Host sanitizer driver for the density-matrix oracle of the C++ CPU simulator (qd_cpu_qsim_mixed_probs).  Built with
// -fsanitize=address,undefined by tests/test_mixed_cpu.py; links the simulator source directly, so no preload is
// needed.  Checks, at n = 2, 5, 8:
//   * the probabilities are >= -1e-15 and sum to 1 within 1e-12, at zero, mixed per-wire and maximal thresholds;
//   * with every threshold 0 they equal qd_cpu_qsim_probs within 1e-12 (two fp64 evaluations of one circuit);
//   * with noise they differ from the noiseless ones, and the same call repeats bit for bit;
//   * out-of-range arguments are refused and leave the output untouched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int qd_cpu_qsim_probs(const float* x, const float* w, double* probs, int B, int n, int L);
extern "C" int qd_cpu_qsim_mixed_probs(const float* x, const float* w, const uint32_t* thr1, const uint32_t* thr2,
                                       double* probs, int B, int n, int L);

static int failures = 0;
static void expect(bool ok, const char* what, int n, int mode) {
  if (!ok) {
    std::printf("FAILED %s (n=%d mode=%d)\n", what, n, mode);
    ++failures;
  }
}

int main() {
  std::mt19937 rng(4321);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const int ns[] = {2, 5, 8};
  for (int n : ns) {
    const int B = 2, L = n == 8 ? 1 : 3, D = 1 << n;
    std::vector<float> x(B * n), w(L * n * 2);
    for (auto& v : x) v = U(rng);
    for (auto& v : w) v = 3.14159f * (1.f + U(rng));
    std::vector<double> p0((size_t)B * D);
    if (qd_cpu_qsim_probs(x.data(), w.data(), p0.data(), B, n, L)) return 2;
    for (int mode = 0; mode < 3; ++mode) {   // 0: no noise; 1: per-wire, with a 0 and a 0.5; 2: every rate 0.5
      std::vector<uint32_t> thr1(n, 0u), thr2(n, 0u);
      for (int q = 0; q < n; ++q) {
        if (mode == 1) {
          thr1[q] = (uint32_t)((0x80000000ull * q) / (n - 1));
          thr2[q] = (uint32_t)((0x80000000ull * (n - 1 - q)) / (n - 1));
        } else if (mode == 2) {
          thr1[q] = thr2[q] = 0x80000000u;
        }
      }
      std::vector<double> p((size_t)B * D, -7.0), p2((size_t)B * D, -7.0);
      if (qd_cpu_qsim_mixed_probs(x.data(), w.data(), thr1.data(), thr2.data(), p.data(), B, n, L)) return 3;
      if (qd_cpu_qsim_mixed_probs(x.data(), w.data(), thr1.data(), thr2.data(), p2.data(), B, n, L)) return 3;
      double away = 0;
      for (int b = 0; b < B; ++b) {
        double s = 0;
        for (int k = 0; k < D; ++k) {
          const double v = p[(size_t)b * D + k];
          expect(v >= -1e-15, "probability >= -1e-15", n, mode);
          expect(v == p2[(size_t)b * D + k], "repeatable", n, mode);
          if (mode == 0) expect(std::fabs(v - p0[(size_t)b * D + k]) <= 1e-12, "zero noise = the state vector", n, mode);
          away = std::fmax(away, std::fabs(v - p0[(size_t)b * D + k]));
          s += v;
        }
        expect(std::fabs(s - 1.0) < 1e-12, "probabilities sum to 1", n, mode);
      }
      if (mode != 0) expect(away > 1e-3, "noise changes the probabilities", n, mode);
    }
  }
  // out-of-range arguments are refused, the output untouched
  float e = 0.f;
  uint32_t thr[16] = {0};
  double d[4] = {-7.0, -7.0, -7.0, -7.0};
  expect(qd_cpu_qsim_mixed_probs(&e, &e, thr, thr, d, 1, 1, 1) != 0, "n = 1 refused", 1, 0);
  expect(qd_cpu_qsim_mixed_probs(&e, &e, thr, thr, d, 1, 9, 1) != 0, "n = 9 refused", 9, 0);
  expect(qd_cpu_qsim_mixed_probs(&e, &e, thr, thr, d, 1, 2, 0) != 0, "L = 0 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_probs(&e, &e, thr, thr, d, 1, 2, 1025) != 0, "2 n L > 4096 refused", 2, 0);
  expect(qd_cpu_qsim_mixed_probs(&e, &e, thr, thr, d, -1, 2, 1) != 0, "B < 0 refused", 2, 0);
  for (double v : d) expect(v == -7.0, "a refused call writes nothing", 0, 0);
  std::printf("qsim_mixed_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
