// Host sanitizer driver for the Pauli-noise pieces of the C++ CPU simulator (qd_cpu_noise_sites, qd_cpu_pauli_frames,
// qd_cpu_qsim_probs_framed, qd_cpu_sample_z_noisy).  Built with -fsanitize=address,undefined by
// tests/test_noise_cpu.py; links the simulator source directly, so no preload is needed.  Checks, at n = 2, 5, 12 with
// T = 1 and 3:
//   * site codes lie in 0 .. 3 / 0 .. 15, frames inside 2^n, framed probabilities are non-negative and sum to 1;
//   * with every threshold 0: no error is drawn, every frame is identity, the framed probabilities equal
//     qd_cpu_qsim_probs and E / counts equal qd_cpu_sample_z bit for bit;
//   * with noise: counts lie in [0, shots], E = (shots - 2 counts) / shots exactly, the same call repeats;
//   * out-of-range arguments are refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int qd_cpu_qsim_probs(const float* x, const float* w, double* probs, int B, int n, int L);
extern "C" int qd_cpu_sample_z(const float* probs, float* E, int32_t* counts, int B, int n, int shots, uint64_t seed,
                               uint64_t ctr);
extern "C" int qd_cpu_noise_sites(uint8_t* sites, const uint32_t* thr1, const uint32_t* thr2, int B, int n, int L,
                                  int T, uint64_t seed, uint64_t ctr);
extern "C" int qd_cpu_pauli_frames(const uint8_t* sites, int32_t* frames, int rows, int n, int L);
extern "C" int qd_cpu_qsim_probs_framed(const float* x, const float* w, const int32_t* frames, double* probs, int B,
                                        int n, int L);
extern "C" int qd_cpu_sample_z_noisy(const float* probs, const int32_t* amask, const uint32_t* thr_ro, float* E,
                                     int32_t* counts, int B, int n, int shots, int T, uint64_t seed, uint64_t ctr);

static int failures = 0;
static void expect(bool ok, const char* what, int n, int T) {
  if (!ok) {
    std::printf("FAILED %s (n=%d T=%d)\n", what, n, T);
    ++failures;
  }
}

int main() {
  const uint64_t seed = 0x1234567800000007ull, ctr = (1ull << 33) + 5;
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const int ns[] = {2, 5, 12}, Ts[] = {1, 3};
  for (int n : ns) {
    for (int T : Ts) {
      const int B = 2, L = 3, D = 1 << n, shots = 24 * T, R = B * T;
      std::vector<float> x(B * n), w(L * n * 2), xr((size_t)R * n);
      for (auto& v : x) v = U(rng);
      for (auto& v : w) v = 3.14159f * (1.f + U(rng));
      for (int r = 0; r < R; ++r)
        for (int q = 0; q < n; ++q) xr[(size_t)r * n + q] = x[(size_t)(r / T) * n + q];
      for (int noisy = 0; noisy < 2; ++noisy) {
        std::vector<uint32_t> thr1(n, noisy ? 0x20000000u : 0u), thr2(n, noisy ? 0x30000000u : 0u);
        std::vector<uint32_t> thr_ro(2 * n, noisy ? 3000u : 0u);
        std::vector<uint8_t> sites((size_t)R * L * n * 2, 0xFF);
        if (qd_cpu_noise_sites(sites.data(), thr1.data(), thr2.data(), B, n, L, T, seed, ctr)) return 2;
        bool any = false;
        for (size_t i = 0; i < sites.size(); ++i) {
          expect(sites[i] <= ((i & 1) ? 15 : 3), "site code in range", n, T);
          any |= sites[i] != 0;
        }
        expect(any == (noisy != 0), noisy ? "errors are drawn" : "zero thresholds draw no error", n, T);
        std::vector<int32_t> frames((size_t)R * L * 2, -1), amask(R);
        if (qd_cpu_pauli_frames(sites.data(), frames.data(), R, n, L)) return 3;
        for (int32_t f : frames) expect(f >= 0 && f < D && (noisy || f == 0), "frame in range", n, T);
        for (int r = 0; r < R; ++r) amask[r] = frames[((size_t)r * L + L - 1) * 2];
        std::vector<double> pd((size_t)R * D), p0((size_t)R * D);
        if (qd_cpu_qsim_probs_framed(xr.data(), w.data(), frames.data(), pd.data(), R, n, L)) return 4;
        if (qd_cpu_qsim_probs(xr.data(), w.data(), p0.data(), R, n, L)) return 4;
        std::vector<float> pf(pd.size());
        for (int r = 0; r < R; ++r) {
          double s = 0;
          for (int k = 0; k < D; ++k) {
            const double p = pd[(size_t)r * D + k];
            expect(p >= 0.0, "probability >= 0", n, T);
            if (!noisy) expect(p == p0[(size_t)r * D + k], "identity frames change nothing", n, T);
            s += p;
            pf[(size_t)r * D + k] = (float)p;
          }
          expect(std::fabs(s - 1.0) < 1e-12, "probabilities sum to 1", n, T);
        }
        std::vector<float> E(B * n), E2(B * n);
        std::vector<int32_t> c(B * n), c2(B * n);
        if (qd_cpu_sample_z_noisy(pf.data(), amask.data(), thr_ro.data(), E.data(), c.data(), B, n, shots, T, seed, ctr))
          return 5;
        if (qd_cpu_sample_z_noisy(pf.data(), amask.data(), thr_ro.data(), E2.data(), nullptr, B, n, shots, T, seed,
                                  ctr))
          return 5;
        for (int i = 0; i < B * n; ++i) {
          expect(c[i] >= 0 && c[i] <= shots, "counts in range", n, T);
          expect(E[i] == (float)(shots - 2 * c[i]) / (float)shots, "E from counts", n, T);
          expect(E[i] == E2[i], "repeatable, null counts accepted", n, T);
        }
        if (!noisy) {   // against the noiseless sampler on the samples' own rows
          std::vector<float> pb((size_t)B * D);
          for (int b = 0; b < B; ++b)
            for (int k = 0; k < D; ++k) pb[(size_t)b * D + k] = pf[(size_t)b * T * D + k];
          if (qd_cpu_sample_z(pb.data(), E2.data(), c2.data(), B, n, shots, seed, ctr)) return 6;
          for (int i = 0; i < B * n; ++i) expect(c[i] == c2[i] && E[i] == E2[i], "zero noise = qd_cpu_sample_z", n, T);
        }
      }
    }
  }
  // out-of-range arguments are refused
  float e = 0.f;
  double d = 0.0;
  int32_t z[8] = {0};
  uint8_t s8[64] = {0};
  uint32_t thr[26] = {0};
  expect(qd_cpu_noise_sites(s8, thr, thr, 1, 13, 1, 1, 0, 0) != 0, "sites: n = 13 refused", 13, 1);
  expect(qd_cpu_noise_sites(s8, thr, thr, 1, 2, 1025, 1, 0, 0) != 0, "sites: 2 n L > 4096 refused", 2, 1);
  expect(qd_cpu_noise_sites(s8, thr, thr, 1, 2, 1, 0, 0, 0) != 0, "sites: T = 0 refused", 2, 0);
  expect(qd_cpu_noise_sites(s8, thr, thr, 1, 2, 1, 1025, 0, 0) != 0, "sites: T > 1024 refused", 2, 1025);
  s8[0] = 4;
  expect(qd_cpu_pauli_frames(s8, z, 1, 2, 1) != 0, "frames: one-qubit code 4 refused", 2, 1);
  s8[0] = 0;
  s8[1] = 16;
  expect(qd_cpu_pauli_frames(s8, z, 1, 2, 1) != 0, "frames: two-qubit code 16 refused", 2, 1);
  z[0] = 4;
  expect(qd_cpu_qsim_probs_framed(&e, &e, z, &d, 1, 2, 1) != 0, "framed: mask outside 2^n refused", 2, 1);
  z[0] = 0;
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 13, 4, 1, 0, 0) != 0, "n = 13 refused", 13, 1);
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 0, 1, 0, 0) != 0, "shots = 0 refused", 2, 1);
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 16, 0, 0, 0) != 0, "T = 0 refused", 2, 0);
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 4100, 1025, 0, 0) != 0, "T > 1024 refused", 2, 1025);
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 16, 3, 0, 0) != 0, "shots % T != 0 refused", 2, 3);
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 18, 3, 0, 0) != 0, "(shots / T) % 4 != 0 refused", 2, 3);
  thr[0] = 65536;
  expect(qd_cpu_sample_z_noisy(&e, z, thr, &e, nullptr, 1, 2, 4, 1, 0, 0) != 0, "readout threshold > 65535 refused", 2,
         1);
  std::printf("qsim_noise_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
