"""Time the parameter-shift kernel (csrc/hip/qsim_pshift.hip) against its composition from the fused shots kernel.

For every configuration (B, n, L, shots) three variants compute the per-sample gradients G (B, P) and dw (P,),
P = 2nL, on the same inputs:
  pshift    qd_qsim_pshift (the state that enters a layer built once per workgroup and kept), then reduce_slab
  composed  what a user could do without it: one qd_qsim_shots_fwd launch over 2P * B rows with 2P groups of shifted
            weights (every state rebuilt from scratch), then the contraction with gE and the sum over the batch in torch
  adjoint   the exact adjoint backward (qsim.hip for n <= 10, qsim_big.hip above) and reduce_slab, for scale
Each variant is captured once as a HIP graph of ITERS back-to-back launches (so the host's launch rate is not what is
timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per launch.  First the kernel's exact-mode G is compared with the
composition's (the exact forward on the same 2P groups of shifted weights).

    python scripts/pshift_timing.py [--rounds 5] [--iters 20] [--out profiles/pshift_timing.txt]
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

CONFIGS = [(2304, 8, 3, 256), (2304, 8, 3, 1024), (256, 12, 3, 1024)]
SEED = 1234


def variants(B, n, L, shots, dev):
    torch.manual_seed(0)
    P = 2 * n * L
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    gE = (torch.rand(B, n) * 2 - 1).to(dev)
    # the composition's inputs: group 2p + s holds w with parameter p shifted by +-pi/2
    ws = w.reshape(1, P).repeat(2 * P, 1)
    idx = torch.arange(P, device=dev)
    ws[2 * idx, idx] += 0.5 * math.pi
    ws[2 * idx + 1, idx] -= 0.5 * math.pi
    ws = ws.view(2 * P, L, n, 2).contiguous()
    xs = x.repeat(2 * P, 1).contiguous()
    Es = torch.empty(2 * P * B, n, device=dev)
    G = torch.empty(B, P, device=dev)
    dw = torch.empty(P, device=dev)
    dx = torch.empty(B, n, device=dev)
    dwa = torch.empty(P, device=dev)
    out = {}

    def contract():
        E = Es.view(P, 2, B, n)
        out["G"] = torch.einsum("pbj,bj->bp", 0.5 * (E[:, 0] - E[:, 1]), gE)
        out["dw"] = out["G"].sum(0)

    def pshift():
        Q.hip_qsim_pshift(x, w, gE, G, shots=shots, seed=SEED)
        Q.reduce_slab(G, dw)

    def composed():
        Q.hip_qsim_shots_fwd(xs, ws, Es, None, shots, SEED, wgroup=B)
        contract()

    def adjoint():
        Q.reduce_slab(Q.hip_qsim_bwd_slab(x, w, gE, dx), dwa)

    # exact mode first: the kernel against the composition on the exact forward
    Q.hip_qsim_pshift(x, w, gE, G, shots=0)
    Q.hip_qsim_fwd(xs, ws, Es, B)
    contract()
    torch.cuda.synchronize()
    err = float(((G - out["G"]).abs() / gE.abs().sum(1, keepdim=True)).max())
    assert err <= 2 * (2e-5 if n <= 10 else 5e-5), f"exact-mode G differs from the composition's: {err:.2e}"
    pshift()
    composed()
    adjoint()
    torch.cuda.synchronize()
    return {"pshift": pshift, "composed": composed, "adjoint": adjoint}, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pshift_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; per-launch time in microseconds, median (min .. max) over {args.rounds} "
             f"rounds of {args.iters} graph-replayed launches, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2} {'shots':>6}  {'pshift':>28}  {'composed':>28}  {'exact adjoint':>24}  "
             f"composed/pshift  ranges apart  max|G_exact-G_composed|/sum|gE|"]
    for B, n, L, shots in CONFIGS:
        fns, err = variants(B, n, L, shots, dev)
        times = time_graphed(fns, args.iters, args.rounds)
        cells = {k: cell(v, 9) for k, v in times.items()}
        ratio = statistics.median(times["composed"]) / statistics.median(times["pshift"])
        apart = "yes" if max(times["pshift"]) < min(times["composed"]) else "NO"
        lines.append(f"{B:>5} {n:>3} {L:>2} {shots:>6}  {cells['pshift']:>28}  {cells['composed']:>28}  "
                     f"{cells['adjoint']:>24}  {ratio:>15.2f}  {apart:>12}  {err:.2e}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
