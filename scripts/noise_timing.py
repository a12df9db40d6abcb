"""Time the noisy finite-shot kernel (csrc/hip/qsim_noise.hip) against the noiseless shots kernel.

For every configuration (B, n, L, shots, T) and noise point four variants run on the same inputs:
  noisy       qd_qsim_noisy_shots_fwd at (B, shots, T) with the noise point's thresholds, the launcher's own grid
              (the workgroups per sample are in the `split` column)
  noisy-1wg   the same with one workgroup per sample forced
  noisy-8     the same with the finest split the shape allows forced (8, 4 or 2 chunks of trajectories per sample)
  no-noise    qd_qsim_shots_fwd at (B, shots): the cost with no noise model
  every-traj  qd_qsim_shots_fwd at (B T rows, shots / T shots): what simulating every trajectory on its own costs
              (its state builds and sampling only: no frame draws, no readout draws, no reduction over T)
Each variant is captured once as a HIP graph of ITERS back-to-back launches (so the host's launch rate is not what is
timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per launch.  With zero thresholds the noisy result is compared with the
no-noise one bit for bit first.

    python scripts/noise_timing.py [--rounds 5] [--iters 200] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed, write_report  # noqa: E402

CONFIGS = [(2304, 8, 3, 1024, 64), (2304, 12, 3, 1024, 16)]
POINTS = {"zero": Q.NoiseModel(), "1e-3/1e-2/2%": Q.NoiseModel(p1=1e-3, p2=1e-2, readout01=0.02, readout10=0.02)}
SEED = 1234


def variants(B, n, L, shots, T, noise, dev):
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    xt = x.repeat_interleave(T, dim=0).contiguous()
    E = torch.empty(B, n, device=dev)
    E0 = torch.empty(B, n, device=dev)
    Et = torch.empty(B * T, n, device=dev)
    frames = torch.empty(B, T, L, 2, device=dev, dtype=torch.int32)

    E1 = torch.empty(B, n, device=dev)

    def noisy():
        Q.hip_qsim_noisy_shots_fwd(x, w, E, None, noise, shots, T, SEED)

    def noisy_1wg():   # (the split is read when the launch is issued, so also when it is captured)
        Q.noise_force_split(1)
        try:
            Q.hip_qsim_noisy_shots_fwd(x, w, E1, None, noise, shots, T, SEED)
        finally:
            Q.noise_force_split(0)

    finest = next(k for k in (8, 4, 2, 1) if T % k == 0)

    def noisy_split():
        Q.noise_force_split(finest)
        try:
            Q.hip_qsim_noisy_shots_fwd(x, w, E1, None, noise, shots, T, SEED)
        finally:
            Q.noise_force_split(0)

    def no_noise():
        Q.hip_qsim_shots_fwd(x, w, E0, None, shots, SEED)

    def every_traj():
        Q.hip_qsim_shots_fwd(xt, w, Et, None, shots // T, SEED)

    Q.hip_qsim_noisy_shots_fwd(x, w, E, None, noise, shots, T, SEED, frames_out=frames)
    noisy_1wg()
    no_noise()
    every_traj()
    torch.cuda.synchronize()
    assert torch.equal(E, E1), "the split changes the result"
    if noise.is_zero:
        assert torch.equal(E, E0), "zero thresholds differ from the noiseless kernel"
    rebuilt = float((frames[:, :, :L - 1] != 0).flatten(2).any(2).float().mean())
    return {"noisy": noisy, "noisy-1wg": noisy_1wg, "noisy-8": noisy_split, "no-noise": no_noise, "every-traj": every_traj}, rebuilt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; per-launch time in microseconds, median (min .. max) over {args.rounds} "
             f"rounds of {args.iters} graph-replayed launches, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2} {'shots':>6} {'T':>4} {'noise':>13} {'split':>5}  {'noisy':>26}  {'noisy-1wg':>26}  {'noisy-8':>26}  {'no-noise (B, shots)':>26}  "
             f"{'every-traj (B T, shots/T)':>30}  noisy/no-noise  every-traj/noisy  rebuilt"]
    for B, n, L, shots, T in CONFIGS:
        for name, noise in POINTS.items():
            fns, rebuilt = variants(B, n, L, shots, T, noise, dev)
            times = time_graphed(fns, args.iters, args.rounds)
            cells = {k: cell(v, 8) for k, v in times.items()}
            med = {k: statistics.median(v) for k, v in times.items()}
            apart = max(times["noisy"]) < min(times["every-traj"]) and max(times["noisy-1wg"]) < min(times["every-traj"])
            lines.append(f"{B:>5} {n:>3} {L:>2} {shots:>6} {T:>4} {name:>13} {Q.noise_split(T, n):>5}  {cells['noisy']:>26}  "
                         f"{cells['noisy-1wg']:>26}  {cells['noisy-8']:>26}  {cells['no-noise']:>26}  "
                         f"{cells['every-traj']:>30}  {med['noisy'] / med['no-noise']:>14.2f}  "
                         f"{med['every-traj'] / med['noisy']:>16.2f}  {rebuilt:7.3f}"
                         f"{'' if apart else '   (ranges overlap)'}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
