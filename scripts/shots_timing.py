"""Time the finite-shot kernels (csrc/hip/qsim_shots.hip) against the exact forward.

For every configuration (B, n, L, shots) three variants run on the same inputs:
  fused      qd_qsim_shots_fwd (state -> probabilities -> shots in one launch)
  two-stage  qd_qsim_probs then qd_sample_z (the probabilities go through HBM)
  exact      the exact <Z> forward of ops.quantum.hip_qsim_fwd (qsim.hip for n <= 10, qsim_big.hip above)
Each variant is captured once as a HIP graph of ITERS back-to-back launches (so the host's launch rate is not what is
timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per launch.  The fused and two-stage outputs are compared bit for bit first.

    python scripts/shots_timing.py [--rounds 5] [--iters 200] [--out FILE]
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

CONFIGS = [(2304, 8, 3, 256), (2304, 8, 3, 1024), (2304, 8, 3, 4096), (2304, 12, 3, 1024)]
SEED = 1234


def variants(B, n, L, shots, dev):
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    E = torch.empty(B, n, device=dev)
    E2 = torch.empty(B, n, device=dev)
    Ex = torch.empty(B, n, device=dev)
    probs = torch.empty(B, 1 << n, device=dev)

    def fused():
        Q.hip_qsim_shots_fwd(x, w, E, None, shots, SEED)

    def two_stage():
        Q.hip_qsim_probs(x, w, probs)
        Q.hip_sample_z(probs, E2, None, n, shots, SEED)

    def exact():
        Q.hip_qsim_fwd(x, w, Ex)

    fused()
    two_stage()
    exact()
    torch.cuda.synchronize()
    assert torch.equal(E, E2), "fused and two-stage results differ"
    return {"fused": fused, "two-stage": two_stage, "exact": exact}, float((E - Ex).abs().max())


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
             f"{'B':>5} {'n':>3} {'L':>2} {'shots':>6}  {'fused':>24}  {'two-stage':>24}  {'exact fwd':>24}  "
             f"two-stage/fused  max|E_shots-E_exact|"]
    for B, n, L, shots in CONFIGS:
        fns, dE = variants(B, n, L, shots, dev)
        times = time_graphed(fns, args.iters, args.rounds)
        cells = {k: cell(v, 8) for k, v in times.items()}
        ratio = statistics.median(times["two-stage"]) / statistics.median(times["fused"])
        lines.append(f"{B:>5} {n:>3} {L:>2} {shots:>6}  {cells['fused']:>24}  {cells['two-stage']:>24}  "
                     f"{cells['exact']:>24}  {ratio:>15.2f}  {dE:.4f}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
