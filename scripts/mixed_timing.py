"""Time the density-matrix kernel (csrc/hip/qsim_mixed.hip) against what it stands in for at evaluation time.

For every configuration (B, n, L) three variants compute E (B, n) on the same inputs:
  mixed     qd_qsim_mixed_fwd: the exact expectation of the noisy device (rho in LDS to n = 7, in the workspace at 8)
  sampled   qd_qsim_noisy_shots_fwd at T = 64 trajectories and 1024 shots: the estimate of that expectation
  exact     the exact noiseless forward (hip_qsim_fwd), for scale
Each variant is captured once as a HIP graph of ITERS back-to-back repetitions (so the host's launch rate is not what
is timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per repetition.

    python scripts/mixed_timing.py [--rounds 5] [--iters 10] [--out profiles/mixed_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed, write_report  # noqa: E402

CONFIGS = [(256, 4, 3), (256, 6, 3), (256, 7, 3), (256, 8, 3), (2304, 8, 3)]
NOISE = Q.NoiseModel(1e-3, 1e-2, 0.02, 0.02)
SHOTS, T = 1024, 64
SEED = 1234


def variants(B, n, L, dev):
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    Em, Es, Ee = (torch.empty(B, n, device=dev) for _ in range(3))

    def mixed():
        Q.hip_qsim_mixed_fwd(x, w, Em, None, NOISE)

    def sampled():
        Q.hip_qsim_noisy_shots_fwd(x, w, Es, None, NOISE, SHOTS, T, SEED)

    def exact():
        Q.hip_qsim_fwd(x, w, Ee)

    mixed()
    sampled()
    exact()
    torch.cuda.synchronize()
    # the sampler estimates what the density matrix computes: per entry within 6 sigma of T trajectory means
    err = float((Em - Es).abs().max())
    assert math.isfinite(err) and err <= 6 / math.sqrt(T), err
    return {"mixed": mixed, "sampled": sampled, "exact": exact}, err, float((Em - Ee).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = ["Density-matrix kernel (csrc/hip/qsim_mixed.hip) against the noisy finite-shot forward at T = 64, 1024 "
             "shots, and the exact noiseless forward; noise 1e-3 / 1e-2 / readout .02: python scripts/mixed_timing.py",
             f"{torch.cuda.get_device_name(0)}; time per forward in microseconds, median (min .. max) over "
             f"{args.rounds} rounds of {args.iters} graph-replayed repetitions, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2}  {'mixed':>28}  {'sampled (T=64, 1024 shots)':>30}  {'exact noiseless':>24}  "
             f"mixed/sampled  ranges apart  mixed/exact  max|E_mixed-E_sampled|  max|E_mixed-E_exact|"]
    for B, n, L in CONFIGS:
        fns, err, away = variants(B, n, L, dev)
        times = time_graphed(fns, args.iters, args.rounds)
        cells = {k: cell(v, 9) for k, v in times.items()}
        med = {k: statistics.median(v) for k, v in times.items()}
        apart = "yes" if (max(times["mixed"]) < min(times["sampled"]) or min(times["mixed"]) > max(times["sampled"])) \
            else "NO"
        lines.append(f"{B:>5} {n:>3} {L:>2}  {cells['mixed']:>28}  {cells['sampled']:>30}  {cells['exact']:>24}  "
                     f"{med['mixed'] / med['sampled']:>13.2f}  {apart:>12}  {med['mixed'] / med['exact']:>11.2f}  "
                     f"{err:>22.4f}  {away:>19.4f}")
        print(lines[-1], flush=True)
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
