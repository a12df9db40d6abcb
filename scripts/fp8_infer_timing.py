"""Time the e4m3 test-time estimator (HIPInference(dtype="fp8")) against the bf16 one, kernel by kernel.

One process, the bf16 and e4m3 variants alternating within a round, at the engine's own shape: a chunk of M = 2304
samples at P128 (K = 4096, N = 2048, E = 3):
  routed FC   ops.fc.gemm_fwd (bf16, cfg 0 and 8) against ops.fc.gemm_fwd_rows_f8 (cfg 0: the non-scaled e4m3 MFMA,
              1: the MX MFMA with unit block scales, 2: the same with producer waves)
  mixed FC    ops.fc.gemm_fwd_mix (cfg 0 and 8) against ops.fc.gemm_fwd_mix_rows_f8 (cfg 0, 1, 2)
  tail        the experts' last launch: the fused BN tail + BN/ReLU apply writing the bf16 operand (qd_bn_apply_tail)
              against the BN tail + the row-quantising apply (qd_bn_stats_finalize_multi + qd_bn_relu_rows_f8)
  estimate    whole HIPInference.estimate / estimate_mixed calls on one chunk, per dtype
Each variant is captured once as a HIP graph of ITERS back-to-back calls, warmed up, and replayed between two HIP
events; the table gives the median and the min .. max over the rounds, per call.  The e4m3 mix with one-hot weights is
first compared with the e4m3 routed forward bit for bit.

    python scripts/fp8_infer_timing.py [--rounds 3] [--iters 400] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import Conv_P128, FC_P128  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc as F  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.conv import BnFwd  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import quantise_rows_e4m3  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed, write_report  # noqa: E402

M, N, K, E = 2304, 2048, 4096, 3
BF = torch.bfloat16


def onehot(expert):
    P = torch.zeros(expert.numel(), E, device=expert.device)
    P[torch.arange(expert.numel(), device=expert.device), expert] = 1.0
    return P


def gemm_variants(dev):
    torch.manual_seed(0)
    A = torch.relu(torch.randn(M * E, K, device=dev)).to(BF)
    Wf = torch.randn(N, K, device=dev) * K ** -0.5
    W, b = Wf.to(BF), torch.randn(N, device=dev).to(BF)
    A8, rs = quantise_rows_e4m3(A)
    W8, cs = quantise_rows_e4m3(Wf)
    expert = torch.randint(0, E, (M,), device=dev)
    P = torch.softmax(4 * torch.randn(M, E, device=dev), 1).contiguous()
    Y = torch.empty(M, N, device=dev, dtype=BF)
    Y2 = torch.empty(M, N, device=dev, dtype=BF)
    fns = {}
    for cfg in (0, 8):
        fns[f"bf16 routed cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd(A, W, b, out=Y, cfg=cfg, expert=expert, n_experts=E)
    for cfg in (0, 1, 2):
        F.gemm_fwd_rows_f8(A8, W8, rs, cs, b, out=Y, cfg=cfg, expert=expert, n_experts=E)
        F.gemm_fwd_mix_rows_f8(A8, W8, rs, cs, b, onehot(expert), out=Y2, cfg=cfg)
        torch.cuda.synchronize()
        assert torch.equal(Y.view(torch.int16), Y2.view(torch.int16)), f"e4m3 cfg {cfg}: one-hot mix differs from routed"
        fns[f"e4m3 routed cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd_rows_f8(A8, W8, rs, cs, b, out=Y, cfg=cfg,
                                                                         expert=expert, n_experts=E)
    for cfg in (0, 8):
        fns[f"bf16 mix cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd_mix(A, W, b, P, out=Y2, cfg=cfg)
    for cfg in (0, 1, 2):
        fns[f"e4m3 mix cfg{cfg}"] = lambda cfg=cfg: F.gemm_fwd_mix_rows_f8(A8, W8, rs, cs, b, P, out=Y2, cfg=cfg)
    return fns


def engines(dev):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(dev).eval() for _ in range(E)]
    fc = FC_P128(128).to(dev).eval()
    return {dt: HIPInference(convs, fc, 128, dev, chunk=M, dtype=dt) for dt in ("bf16", "fp8")}


def tail_variants(eng):
    """The last launch(es) of the experts' eval forward, on the z the stacks hold after one forward."""
    arr = lambda xs: (ctypes.c_void_p * 3)(*[nat.ptr(x) for x in xs])
    fns = {}
    for dt, name in (("bf16", "bf16 tail"), ("fp8", "e4m3 tail")):
        s = eng[dt].conv
        s.forward(eng[dt].x1, training=False)
        m = s.m
        if dt == "bf16":
            def tail(s=s, m=m):
                st = nat.stream_ptr(m.device)
                bnf3 = BnFwd(nat.ptr(s.stats[2]), nat.ptr(m.bn_w[2]), nat.ptr(m.bn_b[2]), nat.ptr(m.run_mean[2]),
                             nat.ptr(m.run_var[2]), nat.ptr(s.st[2]), s.chunks_f, float(s.B * s.HW), m.momentum, m.eps, 0)
                nat.check(s._apply_tail(nat.ptr(s.z[2]), nat.ptr(s.h3), ctypes.byref(bnf3), arr(s.stats), arr(m.bn_w),
                                        arr(m.bn_b), arr(m.run_mean), arr(m.run_var), arr(s.st), s.U, s.E, s.B, s.HW,
                                        s.spb_a, s.chunks_f, 0, None, 0, s.U, None, None, None, st), "bn_apply_tail")
        else:
            def tail(s=s, m=m):
                st = nat.stream_ptr(m.device)
                nat.check(s._fin(3, arr(s.stats), arr(m.bn_w), arr(m.bn_b), arr(m.run_mean), arr(m.run_var), arr(s.st),
                                 s.U, s.chunks_f, s.EC, float(s.B * s.HW), m.momentum, m.eps, 0, None, 0, s.U, st),
                          "bn_tail")
                nat.check(s._rows8(nat.ptr(s.z[2]), nat.ptr(s.st[2]), nat.ptr(s.h8r), nat.ptr(s.rs), None, s.N, s.E,
                                   s.B, s.HW, st), "bn_relu_rows_f8")
        fns[name] = tail
    return fns


def estimate_variants(eng, dev):
    x = torch.randn(M, 2, 16, 8, device=dev)
    expert = torch.randint(0, E, (M,), device=dev)
    P = torch.softmax(4 * torch.randn(M, E, device=dev), 1).contiguous()
    e8 = eng["fp8"]
    assert torch.equal(e8.estimate(x, expert), e8.estimate_mixed(x, onehot(expert))), "e4m3 one-hot estimate_mixed differs"
    rel = float((e8.estimate(x, expert) - eng["bf16"].estimate(x, expert)).norm() / eng["bf16"].estimate(x, expert).norm())
    fns = {}
    for dt, name in (("bf16", "bf16"), ("fp8", "e4m3")):
        fns[f"{name} estimate"] = lambda e=eng[dt]: e.estimate(x, expert)
    for dt, name in (("bf16", "bf16"), ("fp8", "e4m3")):
        fns[f"{name} estimate_mixed"] = lambda e=eng[dt]: e.estimate_mixed(x, P)
    return fns, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; time per call in microseconds, median (min .. max) over {args.rounds} "
             f"rounds of {args.iters} graph-replayed calls, variants alternating within a round",
             f"M = {M} samples, N = {N}, K = {K}, E = {E}; e4m3 one-hot mix checked bit-identical to e4m3 routed first"]
    tg = time_graphed(gemm_variants(dev), args.iters, args.rounds)
    eng = engines(dev)
    tt = time_graphed(tail_variants(eng), args.iters, args.rounds)
    ev, rel = estimate_variants(eng, dev)
    te = time_graphed(ev, max(1, args.iters // 5), args.rounds)
    allv = {**tg, **tt, **te}
    med = {k: statistics.median(v) for k, v in allv.items()}
    for k, v in allv.items():
        lines.append(f"{k:>22}  {cell(v, 9)}")

    def ratio(a, b):
        over = "" if max(allv[a]) < min(allv[b]) or max(allv[b]) < min(allv[a]) else "   (ranges overlap)"
        return f"{a} / {b}: {med[a] / med[b]:.2f}{over}"
    best_r = min((f"e4m3 routed cfg{c}" for c in (0, 1, 2)), key=med.get)
    best_m = min((f"e4m3 mix cfg{c}" for c in (0, 1, 2)), key=med.get)
    lines.append(f"fastest e4m3 routed tile: {best_r}; fastest e4m3 mix tile: {best_m}")
    lines.append(ratio(best_r, min(("bf16 routed cfg0", "bf16 routed cfg8"), key=med.get)))
    lines.append(ratio(best_m, min(("bf16 mix cfg0", "bf16 mix cfg8"), key=med.get)))
    lines.append(ratio("e4m3 tail", "bf16 tail"))
    lines.append(ratio("e4m3 estimate", "bf16 estimate"))
    lines.append(ratio("e4m3 estimate_mixed", "bf16 estimate_mixed"))
    lines.append(f"||H_e4m3 - H_bf16|| / ||H_bf16|| of estimate on these (untrained) models: {rel:.3e}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
