"""Time QuantumNAT post-measurement normalization / quantization in the QSC step (csrc/hip/qsc_postmeas.hip).

(a) The head alone: qd_qsc_head_pm (normalization; normalization + 5 levels with the penalty) against the plain
    qd_qsc_head at (B, n, C) = (2304, 8, 3) and (2304, 12, 3), each captured as a HIP graph of ITERS launches.
(b) The fused measured step of scripts/measured_step_timing.py (noisy_adjoint; n = 8, L = 3, T = 64, 1024 shots at the
    noise point, 9 x 256 samples, QuantumNAT weight noise on, AdamW), captured once as a HIP graph, with
    post-processing off, with normalization, and with normalization + 5 levels.
HIP events around the replays; the variants alternate within a round; median (min .. max) over the rounds.

    python scripts/postmeas_timing.py [--rounds 5] [--iters 20] [--out profiles/postmeas_timing.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace, make_optimizer  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import NoiseModel  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import (alternate, cell, graph_of,  # noqa: E402
                                                                                             write_report)

N, L, T, SHOTS, SEED = 8, 3, 64, 1024, 1234
NOISE = NoiseModel(1e-3, 1e-2, 0.02, 0.02)
_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
POST = {"off": {}, "norm": dict(post_norm=True),
        "norm + 5 levels": dict(post_norm=True, post_quant_levels=5, post_quant_weight=0.1)}


def heads(dev, B, n, C, launches):
    """{variant: graph replay of ``launches`` head launches} on static inputs."""
    lib = nat.hip_lib()
    plain = nat.fn(lib, "qd_qsc_head", [_p] * 10 + [_i] * 5 + [_p])
    pm = nat.fn(lib, "qd_qsc_head_pm", [_p] * 10 + [_i] * 5 + [_p, _p, _f, _f, _i, _f, _f, _p, _p])
    g = torch.Generator().manual_seed(B + n)
    E = (torch.randn(B, n, generator=g) * 0.3).clamp(-1, 1).to(dev)
    wc, bc = torch.randn(C, n, generator=g).to(dev), torch.zeros(C, device=dev)
    lab = torch.randint(0, C, (B,), generator=g).to(dev)
    dE, dwc, dbc, loss = (torch.empty(B, n, device=dev), torch.empty(C, n, device=dev), torch.empty(C, device=dev),
                          torch.empty(1, device=dev))
    rm, rv = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    common = (nat.ptr(E), nat.ptr(wc), nat.ptr(bc), nat.ptr(lab), nat.ptr(dE), nat.ptr(dwc), nat.ptr(dbc), nat.ptr(loss),
              None, None, 0, 0, B, n, C)
    keep = [E, wc, bc, lab, dE, dwc, dbc, loss, rm, rv]

    def many(one):
        def run():
            for _ in range(launches):
                one()
        return run

    st = lambda: nat.stream_ptr(dev)
    runs = {"qd_qsc_head": many(lambda: nat.check(plain(*common, st()), "head")),
            "head_pm norm": many(lambda: nat.check(pm(*common, nat.ptr(rm), nat.ptr(rv), 0.1, 1e-5, 0, 2.0, 0.0, None,
                                                      st()), "head_pm")),
            "head_pm norm + 5 levels": many(lambda: nat.check(pm(*common, nat.ptr(rm), nat.ptr(rv), 0.1, 1e-5, 5, 2.0,
                                                                 0.1, None, st()), "head_pm"))}
    graphs = {k: graph_of(r, warm=1) for k, r in runs.items()}
    return {k: g.replay for k, g in graphs.items()}, (keep, graphs)


def step_world(dev, post):
    torch.manual_seed(0)
    B = 9 * 256
    knobs = dict(diff_method="noisy_adjoint", shots=SHOTS, noise=NOISE, trajectories=T)
    m = QSC_P128(N, L, 3, use_quantumnat=True, use_gradient_pruning=False, **knobs, **post).to(dev).train()
    space = FlatParamSpace(list(m.named_parameters()), dev)
    opt = make_optimizer(space, "adamw", 1e-3, weight_decay=0.01, prune_thr=0.0)
    cstep = ClassifierStep(m, 9, space=space, batch_total=B, hip_kw=dict(knobs, shot_seed=SEED))
    assert cstep.hip is not None and cstep.hip.measured and (cstep.hip.pm is not None) == bool(post)
    x = torch.randn(B, 2, 16, 8, device=dev)
    y = torch.randint(0, 3, (B,), device=dev)

    def run():
        space.zero_grad()
        cstep(x, y)
        opt.step()

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postmeas_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    launches = 50
    lines = ["QuantumNAT post-measurement processing in the QSC step: python scripts/postmeas_timing.py",
             f"{torch.cuda.get_device_name(0)}; HIP events around graph replays, median (min .. max) over {args.rounds} "
             f"rounds, variants alternating within a round",
             f"(a) the head alone, one workgroup; us per launch (graphs of {launches} launches, {args.iters} replays per "
             f"round and variant)"]
    head_diff = {}
    for (B, n, C) in ((2304, 8, 3), (2304, 12, 3)):
        fns, keep = heads(dev, B, n, C, launches)
        t = alternate(fns, args.rounds, args.iters)
        base = statistics.median(t["qd_qsc_head"])
        for k, v in t.items():
            lines.append(f"  ({B}, {n}, {C})  {k:>24}  {cell(v, 9, 3, 1000.0 / launches):>30}  x{statistics.median(v) / base:5.2f}")
            print(lines[-1], flush=True)
            head_diff[(n, k)] = (statistics.median(v) - base) * 1000.0 / launches
        del fns, keep
    lines.append(f"(b) the fused measured step (noisy_adjoint, n = {N}, L = {L}, T = {T}, {SHOTS} shots, 9 x 256 samples), "
                 f"graphed; ms per step ({args.iters} replays per round and variant)")
    graphs = {k: graph_of(step_world(dev, p), warm=3) for k, p in POST.items()}
    t = alternate({k: g.replay for k, g in graphs.items()}, args.rounds, args.iters)
    off = statistics.median(t["off"])
    spread = max(max(v) - min(v) for v in t.values()) * 1000.0
    for k, v in t.items():
        if k == "off":
            lines.append(f"  {k:>16}  {cell(v, 9, 3):>30}  (widest round-to-round spread of the three variants {spread:.1f} us)")
        else:
            gap = (statistics.median(v) - off) * 1000.0
            lines.append(f"  {k:>16}  {cell(v, 9, 3):>30}  on - off {gap:8.1f} us   (head alone, pm - plain: "
                         f"{head_diff[(N, 'head_pm ' + k)]:6.1f} us)")
        print(lines[-1], flush=True)
    lines.append("registers (hipcc -O3 -ffp-contract=fast, packed fp32 off; scripts/resource_usage.py): the step's (8, 3) head "
                 "sits at 128 VGPRs with no scratch -- no slack, a compiler update may tip it into scratch; every C <= 3 "
                 "head up to n = 13 has none; the C = 4 heads at n = 8, 12, 13 spill 36 / 44 / 72 B per lane, n >= 14 more")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
