"""Time the noise-aware adjoint kernel (csrc/hip/qsim_nadj.hip) against the gradient it replaces for simulator training.

For every configuration (B, n, L, T) and noise point three variants compute the per-sample gradients G (B, P) and
dw (P,), P = 2nL, on the same inputs:
  nadj      qd_qsim_noisy_adjoint (one adjoint pass for all trajectories that live on the noiseless state, one per
            rebuilding trajectory), then reduce_slab
  onchip    qd_qsim_noisy_pshift at 1024 shots (2P shifted circuits per sample, each with its own error
            realisations), then reduce_slab
  adjoint   the noiseless adjoint (hip_qsim_bwd_slab) and reduce_slab, for scale
Each variant is captured once as a HIP graph of ITERS back-to-back repetitions (so the host's launch rate is not what
is timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per repetition.  The share of rebuilding trajectories is read from the
frames the kernel reports.

    python scripts/nadj_timing.py [--rounds 5] [--iters 10] [--out profiles/nadj_timing.txt]
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

CONFIGS = [(2304, 8, 3, 64), (256, 12, 3, 16)]
POINTS = [("zero", Q.NoiseModel()), ("1e-3/1e-2/.02", Q.NoiseModel(1e-3, 1e-2, 0.02, 0.02))]
SHOTS = 1024
SEED = 1234
CTR = 5


def variants(B, n, L, T, noise, dev):
    torch.manual_seed(0)
    P = 2 * n * L
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    gE = (torch.rand(B, n) * 2 - 1).to(dev)
    G = torch.empty(B, P, device=dev)
    dw = torch.empty(P, device=dev)
    G1 = torch.empty(B, P, device=dev)
    dw1 = torch.empty(P, device=dev)
    dx = torch.empty(B, n, device=dev)
    dw0 = torch.empty(P, device=dev)
    frames = torch.empty(B, T, L, 2, device=dev, dtype=torch.int32)

    def nadj(frames=None):
        Q.hip_qsim_noisy_adjoint(x, w, gE, G, noise, T, SEED, CTR, frames=frames)
        Q.reduce_slab(G, dw)

    def onchip():
        Q.hip_qsim_noisy_pshift(x, w, gE, G1, shots=SHOTS, seed=SEED, ctr0=CTR, noise=noise, trajectories=T)
        Q.reduce_slab(G1, dw1)

    def adjoint():
        Q.reduce_slab(Q.hip_qsim_bwd_slab(x, w, gE, dx), dw0)

    nadj(frames)
    onchip()
    adjoint()
    torch.cuda.synchronize()
    share = float((frames[:, :, :L - 1] != 0).flatten(2).any(-1).float().mean())
    # the two noisy gradients estimate the same quantity up to the on-chip rule's shot and trajectory noise
    err = float((dw - dw1).abs().max() / B)
    assert math.isfinite(err) and bool(torch.isfinite(G).all())
    if noise.is_zero:
        assert float((G[:, 0:2 * n:2] - dx).abs().max()) <= 2e-4
    return {"nadj": nadj, "onchip": onchip, "adjoint": adjoint}, share, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nadj_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = ["Noise-aware adjoint kernel (csrc/hip/qsim_nadj.hip) against the on-chip gradient at 1024 shots and the "
             "noiseless adjoint: python scripts/nadj_timing.py",
             f"{torch.cuda.get_device_name(0)}; time per gradient in microseconds, median (min .. max) over "
             f"{args.rounds} rounds of {args.iters} graph-replayed repetitions, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2} {'T':>3} {'p1/p2/readout':>14}  {'nadj':>28}  {'onchip (1024 shots)':>30}  "
             f"{'noiseless adjoint':>24}  onchip/nadj  ranges apart  nadj/adjoint  rebuilding share  "
             f"max|dw-dw_onchip|/B"]
    for B, n, L, T in CONFIGS:
        for name, noise in POINTS:
            fns, share, err = variants(B, n, L, T, noise, dev)
            times = time_graphed(fns, args.iters, args.rounds)
            cells = {k: cell(v, 9) for k, v in times.items()}
            ratio = statistics.median(times["onchip"]) / statistics.median(times["nadj"])
            over = statistics.median(times["nadj"]) / statistics.median(times["adjoint"])
            apart = "yes" if max(times["nadj"]) < min(times["onchip"]) else "NO"
            lines.append(f"{B:>5} {n:>3} {L:>2} {T:>3} {name:>14}  {cells['nadj']:>28}  {cells['onchip']:>30}  "
                         f"{cells['adjoint']:>24}  {ratio:>11.2f}  {apart:>12}  {over:>12.2f}  {share:>16.4f}  "
                         f"{err:.2e}")
            print(lines[-1], flush=True)
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
