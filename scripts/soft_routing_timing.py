"""Time soft (posterior-weighted) test-time routing against hard routing on the HIP inference engine.

Two pairs, each from one process with the variants alternating within a round:
  GEMM      ops.fc.gemm_fwd_mix (the dense product over all M E expert rows + the mixing epilogue) against the
            routed ops.fc.gemm_fwd (M rows picked by the expert map), at the engine's own shape M = 2304, N = 2048,
            K = 4096, E = 3, cfg 0 and cfg 8.  The mix runs three times the routed GEMM's MFMA work.
  estimate  HIPInference.estimate_mixed against HIPInference.estimate on one chunk of 2304 samples (gather, the three
            experts' conv stacks -- the same in both -- and the FC).
Each variant is captured once as a HIP graph of ITERS back-to-back calls (so the host's launch rate is not what is
timed), warmed up, and replayed between two events; the table gives the median and the min .. max over the rounds,
per call.  With one-hot weights the mixed results are first compared with the routed ones bit for bit.

    python scripts/soft_routing_timing.py [--rounds 7] [--iters 400] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import Conv_P128, FC_P128  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc as F  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed, write_report  # noqa: E402

M, N, K, E = 2304, 2048, 4096, 3


def onehot(expert):
    P = torch.zeros(expert.numel(), E, device=expert.device)
    P[torch.arange(expert.numel(), device=expert.device), expert] = 1.0
    return P


def gemm_variants(dev):
    torch.manual_seed(0)
    A = torch.randn(M * E, K, device=dev).to(torch.bfloat16)
    W = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, device=dev).to(torch.bfloat16)
    expert = torch.randint(0, E, (M,), device=dev)
    P = torch.softmax(4 * torch.randn(M, E, device=dev), 1).contiguous()
    Yr, Ym = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    fns = {}
    for cfg in (0, 8):
        F.gemm_fwd(A, W, b, out=Yr, cfg=cfg, expert=expert, n_experts=E)
        F.gemm_fwd_mix(A, W, b, onehot(expert), out=Ym, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(Yr.view(torch.int16), Ym.view(torch.int16)), f"cfg {cfg}: one-hot mix differs from the routed forward"
        fns[f"routed cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd(A, W, b, out=Yr, cfg=cfg, expert=expert, n_experts=E)
        fns[f"mix cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd_mix(A, W, b, P, out=Ym, cfg=cfg)
    return fns


def estimate_variants(dev):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(dev).eval() for _ in range(E)]
    fc = FC_P128(128).to(dev).eval()
    eng = HIPInference(convs, fc, 128, dev, chunk=M)
    x = torch.randn(M, 2, 16, 8, device=dev)
    expert = torch.randint(0, E, (M,), device=dev)
    P = torch.softmax(4 * torch.randn(M, E, device=dev), 1).contiguous()
    assert torch.equal(eng.estimate(x, expert), eng.estimate_mixed(x, onehot(expert))), "one-hot estimate_mixed differs"
    return {"estimate": lambda: eng.estimate(x, expert), "estimate_mixed": lambda: eng.estimate_mixed(x, P)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; time per call in microseconds, median (min .. max) over {args.rounds} "
             f"rounds of {args.iters} graph-replayed calls, variants alternating within a round",
             f"M = {M} samples, N = {N}, K = {K}, E = {E}; one-hot weights checked bit-identical to the routed path first"]
    tg = time_graphed(gemm_variants(dev), args.iters, args.rounds)
    te = time_graphed(estimate_variants(dev), max(1, args.iters // 5), args.rounds)
    med = {k: statistics.median(v) for k, v in {**tg, **te}.items()}
    for k, v in {**tg, **te}.items():
        lines.append(f"{k:>16}  {cell(v, 9)}")
    for cfg in (0, 8):
        r, m = tg[f"routed cfg{cfg}"], tg[f"mix cfg{cfg}"]
        lines.append(f"mix / routed GEMM, cfg {cfg}: {med[f'mix cfg{cfg}'] / med[f'routed cfg{cfg}']:.2f}"
                     f"   ({2 * M * E * N * K / med[f'mix cfg{cfg}'] * 1e-6:.0f} against "
                     f"{2 * M * N * K / med[f'routed cfg{cfg}'] * 1e-6:.0f} TFLOP/s)"
                     f"{'' if max(r) < min(m) else '   (ranges overlap)'}")
    lines.append(f"estimate_mixed / estimate: {med['estimate_mixed'] / med['estimate']:.2f}"
                 f"{'' if max(te['estimate']) < min(te['estimate_mixed']) else '   (ranges overlap)'}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
