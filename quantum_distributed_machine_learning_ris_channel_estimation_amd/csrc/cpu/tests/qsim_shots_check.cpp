// Host sanitizer driver for the finite-shot pieces of the C++ CPU simulator (qd_cpu_qsim_probs, qd_cpu_sample_z,
// qd_cpu_philox4x32).  Built with -fsanitize=address,undefined by tests/test_shots_cpu.py; links the simulator
// source directly, so no preload is needed.  Checks, at n = 2, 6, 12 and shots = 1, 63, 257:
//   * the Philox4x32-10 known answers (Random123's kat_vectors);
//   * probabilities are non-negative and sum to 1;
//   * counts lie in [0, shots], E = (shots - 2 counts) / shots exactly, and the same (seed, counter) repeats;
//   * one-hot distributions give the signs of the index's bits; a null counts pointer is accepted.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int qd_cpu_qsim_probs(const float* x, const float* w, double* probs, int B, int n, int L);
extern "C" int qd_cpu_sample_z(const float* probs, float* E, int32_t* counts, int B, int n, int shots, uint64_t seed,
                               uint64_t ctr);
extern "C" void qd_cpu_philox4x32(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);

static int failures = 0;
static void expect(bool ok, const char* what, int n, int shots) {
  if (!ok) {
    std::printf("FAILED %s (n=%d shots=%d)\n", what, n, shots);
    ++failures;
  }
}

int main() {
  const uint32_t kat[3][10] = {
      {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
      {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu,
       0xa20bc7c6u, 0x6d5451fdu},
      {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu,
       0x5001e420u, 0x24126ea1u}};
  for (const auto& v : kat) {
    uint32_t out[4];
    qd_cpu_philox4x32(v, v + 4, out);
    for (int i = 0; i < 4; ++i) expect(out[i] == v[6 + i], "philox known answer", 0, 0);
  }

  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const int ns[] = {2, 6, 12}, shot_list[] = {1, 63, 257};
  for (int n : ns) {
    const int B = 3, L = 2, D = 1 << n;
    std::vector<float> x(B * n), w(L * n * 2);
    for (auto& v : x) v = U(rng);
    for (auto& v : w) v = 3.14159f * (1.f + U(rng));
    std::vector<double> pd((size_t)B * D);
    if (qd_cpu_qsim_probs(x.data(), w.data(), pd.data(), B, n, L)) return 2;
    std::vector<float> pf(pd.size());
    for (int b = 0; b < B; ++b) {
      double s = 0;
      for (int k = 0; k < D; ++k) {
        const double p = pd[(size_t)b * D + k];
        expect(p >= 0.0, "probability >= 0", n, 0);
        s += p;
        pf[(size_t)b * D + k] = (float)p;
      }
      expect(std::fabs(s - 1.0) < 1e-12, "probabilities sum to 1", n, 0);
    }
    for (int shots : shot_list) {
      std::vector<float> E(B * n), E2(B * n);
      std::vector<int32_t> c(B * n), c2(B * n);
      if (qd_cpu_sample_z(pf.data(), E.data(), c.data(), B, n, shots, 0x1234567800000007ull, (1ull << 33) + 5)) return 3;
      if (qd_cpu_sample_z(pf.data(), E2.data(), c2.data(), B, n, shots, 0x1234567800000007ull, (1ull << 33) + 5))
        return 3;
      for (int i = 0; i < B * n; ++i) {
        expect(c[i] >= 0 && c[i] <= shots, "counts in range", n, shots);
        expect(E[i] == (float)(shots - 2 * c[i]) / (float)shots, "E from counts", n, shots);
        expect(c[i] == c2[i] && E[i] == E2[i], "repeatable", n, shots);
      }
      // one-hot rows at 0, 2^n - 1 and 5 % 2^n
      const int hot[3] = {0, D - 1, 5 % D};
      std::vector<float> oh((size_t)3 * D, 0.f);
      for (int b = 0; b < 3; ++b) oh[(size_t)b * D + hot[b]] = 1.f;
      if (qd_cpu_sample_z(oh.data(), E.data(), nullptr, 3, n, shots, 7, 0)) return 4;
      for (int b = 0; b < 3; ++b)
        for (int i = 0; i < n; ++i)
          expect(E[b * n + i] == (((hot[b] >> i) & 1) ? -1.f : 1.f), "one-hot signs", n, shots);
    }
  }
  // out-of-range arguments are refused
  float e;
  expect(qd_cpu_sample_z(&e, &e, nullptr, 1, 13, 1, 0, 0) != 0, "n = 13 refused", 13, 1);
  expect(qd_cpu_sample_z(&e, &e, nullptr, 1, 2, 0, 0, 0) != 0, "shots = 0 refused", 2, 0);
  expect(qd_cpu_sample_z(&e, &e, nullptr, 1, 2, (1 << 20) + 1, 0, 0) != 0, "shots > 2^20 refused", 2, (1 << 20) + 1);
  std::printf("qsim_shots_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
