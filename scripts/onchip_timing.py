"""Time the on-chip gradient kernel (csrc/hip/qsim_onchip.hip) against its composition from the noisy shots kernel.

For every configuration (B, n, L, shots, T) and noise point three variants compute the per-sample gradients G (B, P)
and dw (P,), P = 2nL, on the same inputs:
  onchip    qd_qsim_noisy_pshift (the state that enters a layer built once per workgroup and kept; per circuit one
            noiseless state for the error-free trajectories, the others rebuilt), then reduce_slab
  composed  what a user could do without it: 2P launches of qd_qsim_noisy_shots_fwd, one per shifted circuit with its
            shifted weights and its counter c + ((1 + 2p + s) << 48), then the contraction with gE and the sum over
            the batch in torch
  pshift    the noiseless qd_qsim_pshift at the same shots and reduce_slab, for scale
Each variant is captured once as a HIP graph of ITERS back-to-back repetitions (so the host's launch rate is not what
is timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per repetition.  First the kernel's expectations are compared with the
composition's: the same frames and shot streams, so they differ only where the two kernels' fp32 probabilities round
a CDF word differently.

    python scripts/onchip_timing.py [--rounds 5] [--iters 10] [--out profiles/onchip_timing.txt]
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

CONFIGS = [(2304, 8, 3, 1024, 64), (256, 12, 3, 1024, 16)]
POINTS = [("zero", Q.NoiseModel()), ("1e-3/1e-2/.02", Q.NoiseModel(1e-3, 1e-2, 0.02, 0.02))]
SEED = 1234
CTR = 5


def variants(B, n, L, shots, T, noise, dev):
    torch.manual_seed(0)
    P = 2 * n * L
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    gE = (torch.rand(B, n) * 2 - 1).to(dev)
    # the composition's inputs: circuit 2p + s holds w with parameter p shifted by +-pi/2
    ws = w.reshape(1, P).repeat(2 * P, 1)
    idx = torch.arange(P, device=dev)
    ws[2 * idx, idx] += 0.5 * math.pi
    ws[2 * idx + 1, idx] -= 0.5 * math.pi
    ws = ws.view(2 * P, L, n, 2).contiguous()
    Es = torch.empty(2 * P, B, n, device=dev)
    G = torch.empty(B, P, device=dev)
    Epm = torch.empty(B, P, 2, n, device=dev)
    dw = torch.empty(P, device=dev)
    G0 = torch.empty(B, P, device=dev)
    dw0 = torch.empty(P, device=dev)
    out = {}

    def onchip(Epm=None):
        Q.hip_qsim_noisy_pshift(x, w, gE, G, Epm, shots=shots, seed=SEED, ctr0=CTR, noise=noise, trajectories=T)
        Q.reduce_slab(G, dw)

    def composed():
        for c in range(2 * P):
            Q.hip_qsim_noisy_shots_fwd(x, ws[c], Es[c], None, noise, shots, T, SEED,
                                       Q.pshift_counter(CTR, c >> 1, c & 1))
        E = Es.view(P, 2, B, n)
        out["G"] = torch.einsum("pbj,bj->bp", 0.5 * (E[:, 0] - E[:, 1]), gE)
        out["dw"] = out["G"].sum(0)

    def pshift():
        Q.hip_qsim_pshift(x, w, gE, G0, shots=shots, seed=SEED, ctr0=CTR)
        Q.reduce_slab(G0, dw0)

    onchip(Epm)
    composed()
    pshift()
    torch.cuda.synchronize()
    same = float((Epm.permute(1, 2, 0, 3).reshape(2 * P, B, n) == Es).float().mean())
    err = float(((G - out["G"]).abs() / gE.abs().sum(1, keepdim=True)).max())
    assert same >= 0.9 and err <= 0.05, f"the kernel and the composition disagree: {same:.4f} equal, max {err:.2e}"
    return {"onchip": onchip, "composed": composed, "pshift": pshift}, same, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onchip_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; time per gradient in microseconds, median (min .. max) over {args.rounds} "
             f"rounds of {args.iters} graph-replayed repetitions, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2} {'shots':>6} {'T':>3} {'p1/p2/readout':>14}  {'onchip':>30}  {'composed':>30}  "
             f"{'noiseless pshift':>28}  composed/onchip  ranges apart  onchip/pshift  E entries equal  "
             f"max|G-G_composed|/sum|gE|"]
    for B, n, L, shots, T in CONFIGS:
        for name, noise in POINTS:
            fns, same, err = variants(B, n, L, shots, T, noise, dev)
            times = time_graphed(fns, args.iters, args.rounds)
            cells = {k: cell(v, 9) for k, v in times.items()}
            ratio = statistics.median(times["composed"]) / statistics.median(times["onchip"])
            over = statistics.median(times["onchip"]) / statistics.median(times["pshift"])
            apart = "yes" if max(times["onchip"]) < min(times["composed"]) else "NO"
            lines.append(f"{B:>5} {n:>3} {L:>2} {shots:>6} {T:>3} {name:>14}  {cells['onchip']:>30}  "
                         f"{cells['composed']:>30}  {cells['pshift']:>28}  {ratio:>15.2f}  {apart:>12}  {over:>13.2f}  "
                         f"{same:>15.5f}  {err:.2e}")
            print(lines[-1], flush=True)
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
