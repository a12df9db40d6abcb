"""Time the low-latency estimate path (HIPInference.session, csrc/hip/gemm_skinny.hip) against what the tiled engine
offers for the same request.

One process, the variants alternating within a round, P128 (N = 2048, K = 4096, E = 3):
  FC alone       ops.fc.gemm_fwd_skinny* at M = 1, 8, 16 against the tiled forwards at their smallest shapes: gemm_fwd
                 (M = 144 routed rows -- it tiles its output rows --, cfg 0 and 8), gemm_fwd_mix (M = 48, cfg 0 and 8),
                 gemm_fwd_rows_f8 (M = 144, cfg 0-2) and gemm_fwd_mix_rows_f8 (M = 48: 144 rows, cfg 0-2).  Every variant is a graph of ITERS
                 calls.  "warm": the same weight every call (it stays in the Infinity Cache); "cold": the calls cycle
                 over enough weight copies to exceed 256 MiB.  The achieved weight bytes per second are given beside
                 the 6.3 TB/s of a measured device copy.
  whole request  session.run(x) at batch 1, 8, 16 (quantum / classical, hard / soft, bf16 / fp8; one graph replay,
                 issued from Python like any call) against classify + estimate / estimate_mixed on an engine at its
                 smallest chunk (bf16 soft: 48; bf16 hard and fp8: 144), eager, as a user would call it.  ITERS / 4 calls between two HIP events.
Per pair the table says whether the new path's slowest round beats the old path's fastest round.

    python scripts/session_timing.py [--rounds 3] [--iters 400] [--out profiles/session_timing.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,  # noqa: E402
                                                                                             QSC_P128, SC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc as F  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import quantise_rows_e4m3  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import (alternate, cell, graph_of,  # noqa: E402
                                                                                           write_report)

N, K, E = 2048, 4096, 3
BF = torch.bfloat16
COPY_RATE = 6.3e12
MS = (1, 8, 16)
_KEEP = []   # (graph executables live until exit: utils/profiling.py's rule)


def fc_variants(dev, cold: bool):
    """{name: (callable(i) of call i, weight bytes per call)}; call i uses weight copy i % copies."""
    torch.manual_seed(0)
    A = torch.relu(torch.randn(144, K, device=dev)).to(BF)
    Wf = torch.randn(N, K, device=dev) * K ** -0.5
    b = torch.randn(N, device=dev).to(BF)
    A8, rs = quantise_rows_e4m3(A)
    W8_, cs = quantise_rows_e4m3(Wf)
    n16 = (256 * 2 ** 20) // (N * K * 2) + 1 if cold else 1
    n8 = (256 * 2 ** 20) // (N * K) + 1 if cold else 1
    W = [Wf.to(BF).clone() for _ in range(n16)]
    W8 = [W8_.clone() for _ in range(n8)]
    ex = {m: torch.randint(0, E, (m,), device=dev) for m in MS + (48, 144)}
    P = {m: torch.softmax(4 * torch.randn(m, E, device=dev), 1).contiguous() for m in MS + (48,)}
    Y = torch.empty(144, N, device=dev, dtype=BF)
    ws = F.gemm_skinny_workspace(N, K, dev)
    v = {}
    for m in MS:
        v[f"bf16 routed skinny M={m}"] = (lambda i, m=m: F.gemm_fwd_skinny(A[:m * E], W[i % n16], b, out=Y[:m], expert=ex[m], n_experts=E, ws=ws), 2)
    A3 = torch.cat([A, A, A]).contiguous()
    for cfg in (0, 8):   # (the routed forward tiles its M OUTPUT rows: 144 is its smallest M)
        v[f"bf16 routed tiled M=144 cfg{cfg}"] = (lambda i, cfg=cfg: F.gemm_fwd(A3, W[i % n16], b, out=Y, cfg=cfg, expert=ex[144], n_experts=E), 2)
    for m in MS:
        v[f"bf16 mix skinny M={m}"] = (lambda i, m=m: F.gemm_fwd_skinny_mix(A[:m * E], W[i % n16], b, P[m], out=Y[:m], ws=ws), 2)
    for cfg in (0, 8):
        v[f"bf16 mix tiled M=48 cfg{cfg}"] = (lambda i, cfg=cfg: F.gemm_fwd_mix(A, W[i % n16], b, P[48], out=Y[:48], cfg=cfg), 2)
    for m in MS:
        v[f"e4m3 routed skinny M={m}"] = (lambda i, m=m: F.gemm_fwd_skinny_rows_f8(A8[:m * E], W8[i % n8], rs, cs, b, out=Y[:m], expert=ex[m], n_experts=E, ws=ws), 1)
    A8x = torch.cat([A8, A8, A8]).contiguous()
    rsx = torch.cat([rs, rs, rs]).contiguous()
    for cfg in (0, 1, 2):
        v[f"e4m3 routed tiled M=144 cfg{cfg}"] = (lambda i, cfg=cfg: F.gemm_fwd_rows_f8(A8x, W8[i % n8], rsx, cs, b, out=Y, cfg=cfg, expert=ex[144], n_experts=E), 1)
    for m in MS:
        v[f"e4m3 mix skinny M={m}"] = (lambda i, m=m: F.gemm_fwd_skinny_mix_rows_f8(A8[:m * E], W8[i % n8], rs, cs, b, P[m], out=Y[:m], ws=ws), 1)
    for cfg in (0, 1, 2):
        v[f"e4m3 mix tiled M=48 cfg{cfg}"] = (lambda i, cfg=cfg: F.gemm_fwd_mix_rows_f8(A8, W8[i % n8], rs, cs, b, P[48], out=Y[:48], cfg=cfg), 1)
    return v


def time_fc(dev, cold, iters, rounds):
    v = fc_variants(dev, cold)
    graphs = {}
    for name, (f, _) in v.items():
        f(0)
        torch.cuda.synchronize()
        ctr = iter(range(10 ** 9))
        graphs[name] = graph_of(lambda f=f, ctr=ctr: f(next(ctr)), iters)
    _KEEP.append(graphs)
    t = alternate({k: g.replay for k, g in graphs.items()}, rounds, 1, 1e3 / iters)
    return t, {k: b * N * K for k, (_, b) in v.items()}


def models(dev):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(dev).eval() for _ in range(E)]
    return convs, FC_P128(128).to(dev).eval(), SC_P128(128).to(dev).eval(), \
        QSC_P128(8, 3, 3, False, False, 128).to(dev).eval()


def request_variants(dev):
    convs, fc, sc, qsc = models(dev)
    mk = lambda dt, c: HIPInference(convs, fc, 128, dev, chunk=c, sc=sc, qsc=qsc, dtype=dt)
    e8 = mk("fp8", 144)
    eng = {("bf16", "hard"): mk("bf16", 144), ("bf16", "soft"): mk("bf16", 48), ("fp8", "hard"): e8, ("fp8", "soft"): e8}
    x = torch.randn(16, 2, 16, 8, device=dev)
    fns, launches = {}, {}
    for dt in ("bf16", "fp8"):
        for which in ("quantum", "classical"):
            for routing in ("hard", "soft"):
                for m in MS:
                    s = eng[dt, routing].session(m, which=which, routing=routing)
                    key = f"{dt} {which} {routing} batch={m}"
                    fns[key + " session"] = lambda s=s, m=m: s.run(x[:m])
                    launches[f"{dt} {which} {routing}"] = s.launches

                    def old(e=eng[dt, routing], m=m, which=which, routing=routing):
                        pred, logp = e.classify(x[:m], which, return_logp=True)
                        return e.estimate(x[:m], pred) if routing == "hard" else e.estimate_mixed(x[:m], torch.exp(logp))
                    fns[key + " engine"] = old
    return fns, launches


def verdict(new, old):
    return "new slowest < old fastest" if max(new) < min(old) else "NOT MET (ranges overlap or new is slower)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"{torch.cuda.get_device_name(0)}; microseconds per call, median (min .. max) over {args.rounds} rounds, "
             f"variants alternating within a round", f"N = {N}, K = {K}, E = {E}", ""]
    for cold in (False, True):
        t, nbytes = time_fc(dev, cold, args.iters, args.rounds)
        lines.append(f"FC alone, {'cold (weight copies cycling over > 256 MiB)' if cold else 'warm (one weight, Infinity-Cache resident)'}:"
                     f" graphs of {args.iters} calls; weight TB/s at the median (device copy: {COPY_RATE / 1e12:.1f})")
        for k, v in t.items():
            med = sorted(v)[len(v) // 2]
            lines.append(f"  {k:>34}  {cell(v, 8, 2)}   {nbytes[k] / (med * 1e-6) / 1e12:5.2f} TB/s")
        for fmt, form, cfgs, mt in (("bf16", "routed", (0, 8), 144), ("bf16", "mix", (0, 8), 48),
                                    ("e4m3", "routed", (0, 1, 2), 144), ("e4m3", "mix", (0, 1, 2), 48)):
            olds = [f"{fmt} {form} tiled M={mt} cfg{c}" for c in cfgs]
            best = min(olds, key=lambda k: min(t[k]))
            for m in MS:
                lines.append(f"  pair {fmt} {form} skinny M={m} vs {best}: {verdict(t[f'{fmt} {form} skinny M={m}'], t[best])}")
        lines.append("")
        torch.cuda.empty_cache()
    fns, launches = request_variants(dev)
    it = max(1, args.iters // 4)
    t = alternate(fns, args.rounds, it, 1e3)
    lines.append(f"whole request: session.run (one graph replay) against classify + estimate / estimate_mixed (eager, smallest chunk); "
                 f"{it} calls between two events")
    for k in list(fns):
        if k.endswith(" session"):
            o = k[:-len(" session")] + " engine"
            lines.append(f"  {k[:-8]:>34}  session {cell(t[k], 8, 1)}   engine {cell(t[o], 8, 1)}   {verdict(t[k], t[o])}")
    lines.append("")
    lines.append("launches of one session.run, in order:")
    for k, v in launches.items():
        lines.append(f"  {k} ({len(v)}): " + "; ".join(v))
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
