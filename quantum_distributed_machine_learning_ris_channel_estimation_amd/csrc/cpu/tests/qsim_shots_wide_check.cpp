// Host sanitizer driver for the wide shot sampler of the C++ CPU simulator (qd_cpu_sample_z_wide, 2 <= n <= 16: the
// oracle of csrc/hip/qsim_stream_shots.hip).  Built with -fsanitize=address,undefined by
// tests/test_shots_stream_cpu.py; links the simulator source directly, so no preload is needed.  Checks, at n = 13, 16
// and shots = 1, 63, 257:
//   * counts lie in [0, shots], E = (shots - 2 counts) / shots exactly, and the same (seed, counter) repeats;
//   * one-hot rows at outcome 0, D - 1, 4095 and 4096 (either side of the first 4096-outcome block's end) give the
//     signs of the index's bits; a null counts pointer is accepted;
//   * an all-zero row gives outcome D - 1 for every shot;
//   * n = 17, shots = 0 and shots = 2^20 + 1 are refused.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int qd_cpu_sample_z_wide(const float* probs, float* E, int32_t* counts, int B, int n, int shots,
                                    uint64_t seed, uint64_t ctr);

static int failures = 0;
static void expect(bool ok, const char* what, int n, int shots) {
  if (!ok) {
    std::printf("FAILED %s (n=%d shots=%d)\n", what, n, shots);
    ++failures;
  }
}

int main() {
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  const int ns[] = {13, 16}, shot_list[] = {1, 63, 257};
  for (int n : ns) {
    const int B = 2, D = 1 << n;
    std::vector<float> pf((size_t)B * D);
    for (int b = 0; b < B; ++b) {
      double s = 0;
      for (int k = 0; k < D; ++k) s += (pf[(size_t)b * D + k] = U(rng));
      for (int k = 0; k < D; ++k) pf[(size_t)b * D + k] = (float)(pf[(size_t)b * D + k] / s);
    }
    for (int shots : shot_list) {
      std::vector<float> E(5 * n), E2(B * n);
      std::vector<int32_t> c(5 * n), c2(B * n);
      const uint64_t seed = 0x1234567800000007ull, ctr = (1ull << 33) + 5;
      if (qd_cpu_sample_z_wide(pf.data(), E.data(), c.data(), B, n, shots, seed, ctr)) return 3;
      if (qd_cpu_sample_z_wide(pf.data(), E2.data(), c2.data(), B, n, shots, seed, ctr)) return 3;
      for (int i = 0; i < B * n; ++i) {
        expect(c[i] >= 0 && c[i] <= shots, "counts in range", n, shots);
        expect(E[i] == (float)(shots - 2 * c[i]) / (float)shots, "E from counts", n, shots);
        expect(c[i] == c2[i] && E[i] == E2[i], "repeatable", n, shots);
      }
      // one-hot rows at 0, D - 1, 4095 and 4096; the fifth row is all zero
      const int hot[4] = {0, D - 1, 4095, 4096};
      std::vector<float> oh((size_t)5 * D, 0.f);
      for (int b = 0; b < 4; ++b) oh[(size_t)b * D + hot[b]] = 1.f;
      if (qd_cpu_sample_z_wide(oh.data(), E.data(), nullptr, 5, n, shots, 7, 0)) return 4;
      for (int b = 0; b < 4; ++b)
        for (int i = 0; i < n; ++i)
          expect(E[b * n + i] == (((hot[b] >> i) & 1) ? -1.f : 1.f), "one-hot signs", n, shots);
      if (qd_cpu_sample_z_wide(oh.data() + (size_t)4 * D, E.data(), c.data(), 1, n, shots, 7, 0)) return 4;
      for (int i = 0; i < n; ++i) expect(c[i] == shots && E[i] == -1.f, "all-zero row gives D - 1", n, shots);
    }
  }
  // out-of-range arguments are refused
  float e;
  expect(qd_cpu_sample_z_wide(&e, &e, nullptr, 1, 17, 1, 0, 0) != 0, "n = 17 refused", 17, 1);
  expect(qd_cpu_sample_z_wide(&e, &e, nullptr, 1, 13, 0, 0, 0) != 0, "shots = 0 refused", 13, 0);
  expect(qd_cpu_sample_z_wide(&e, &e, nullptr, 1, 13, (1 << 20) + 1, 0, 0) != 0, "shots > 2^20 refused", 13,
         (1 << 20) + 1);
  std::printf("qsim_shots_wide_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
