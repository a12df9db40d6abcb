"""Time the QSC training step under shots and device noise: the fused, graph-captured step (ops/qsc.py QSCStepHIP's
measured modes) against the module path, and the on-chip step with and without QOC gradient pruning (ops/qoc.py).

(a) One whole step (zero_grad, forward, backward, AdamW) at 9 streams x 256 samples, n = 8, L = 3, 1024 shots over
    T = 64 trajectories at the noise point p1 = 1e-3, p2 = 1e-2, readout 0.02 / 0.02, QuantumNAT weight noise on,
    for diff_method = noisy_adjoint and adjoint:
      fused    ClassifierStep with the fused step, captured once as a HIP graph; ITERS replays between two events
      module   ClassifierStep through the model's own forward and autograd, as the runner's qsc_step=module trains
               it: it cannot be captured (host-side tensor work per step), so ITERS eager steps between two events
(b) The on_chip step in the fused, graphed path at 256 samples (one stream), same settings: qsc_prune_ratio 0 against
    0.5 (accum 1, window 2), every replay timed on its own over whole accumulate / prune periods; the shifted
    circuits each step ran are counted from the mask it ran under (a masked layer-0 RY column still runs, for dx).
    The same at 9 x 256 samples, where the shifted circuits' workgroups fill the GPU many times over.
The variants alternate within a round; the table gives the median and min .. max over the rounds.

    python scripts/measured_step_timing.py [--rounds 5] [--iters 10] [--out profiles/measured_step_timing.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace, make_optimizer  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qoc import QOCPruner  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import NoiseModel  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import (alternate, cell, graph_of,  # noqa: E402
                                                                                             timed, write_report)

N, L, T, SHOTS, SEED = 8, 3, 64, 1024, 1234
NOISE = NoiseModel(1e-3, 1e-2, 0.02, 0.02)


def world(dev, streams, per_stream, diff_method, fused, prune_ratio=None):
    """(run, pruner): one training step on static inputs, through the fused step or the module path."""
    torch.manual_seed(0)
    B = streams * per_stream
    knobs = dict(diff_method=diff_method, shots=SHOTS, noise=NOISE, trajectories=T)
    m = QSC_P128(N, L, 3, use_quantumnat=True, use_gradient_pruning=False, **knobs).to(dev).train()
    m.qlayer.manual_shot_seed(SEED)
    space = FlatParamSpace(list(m.named_parameters()), dev)
    opt = make_optimizer(space, "adamw", 1e-3, weight_decay=0.01, prune_thr=0.0)
    pruner = QOCPruner(2 * N * L, prune_ratio, 1, 2, seed=SEED, device=dev) if prune_ratio is not None else None
    if fused:
        kw = dict(knobs, shot_seed=SEED, shift_mask=pruner.mask if pruner is not None else None)
        cstep = ClassifierStep(m, streams, space=space, batch_total=B, hip_kw=kw)
        assert cstep.hip is not None and cstep.hip.measured
    else:
        cstep = ClassifierStep(m, streams)
        assert cstep.hip is None
    x = torch.randn(B, 2, 16, 8, device=dev)
    y = torch.randint(0, 3, (B,), device=dev)

    def run():
        space.zero_grad()
        cstep(x, y)
        if pruner is not None:
            pruner.update(m.qlayer.weights.grad)
        opt.step()

    return run, pruner


def part_a(dev, rounds, iters, lines):
    lines.append(f"(a) whole step, 9 x 256 samples, n = {N}, L = {L}, T = {T}, {SHOTS} shots, noise point; ms per step")
    lines.append(f"{'diff_method':>14}  {'fused + graphed':>30}  {'module path (eager)':>30}  module/fused  ranges apart")
    for dm in ("noisy_adjoint", "adjoint"):
        fused, _ = world(dev, 9, 256, dm, True)
        module, _ = world(dev, 9, 256, dm, False)
        g = graph_of(fused, warm=3)
        times = alternate({"fused": g.replay, "module": module}, rounds, iters)
        ratio = statistics.median(times["module"]) / statistics.median(times["fused"])
        apart = "yes" if max(times["fused"]) < min(times["module"]) else "NO"
        lines.append(f"{dm:>14}  {cell(times['fused'], 9, 3):>30}  {cell(times['module'], 9, 3):>30}  {ratio:>12.2f}  {apart:>12}")
        print(lines[-1], flush=True)


def circuits(mask):
    """Shifted circuits per sample a step runs under ``mask``: two per parameter that is kept or carries dx."""
    keep = mask.bool().cpu()
    p = torch.arange(keep.numel())
    return 2 * int((keep | ((p < 2 * N) & (p % 2 == 0))).sum())


def part_b(dev, rounds, periods, lines, streams=1):
    P = 2 * N * L
    lines.append(f"(b) on_chip step, fused + graphed, {streams} x 256 samples, same settings; ms per step over {periods} "
                 f"periods of 3 steps (1 accumulating, 2 pruned); circuits = shifted circuits per sample, of {2 * P}")
    lines.append(f"{'ratio':>6}  {'all steps':>30}  {'accumulating steps':>30}  {'pruned steps':>30}  "
                 f"mean circuits  circuits in pruned steps")
    worlds = {r: world(dev, streams, 256, "on_chip", True, prune_ratio=r) for r in (0.0, 0.5)}
    graphs = {r: graph_of(run, warm=3) for r, (run, _) in worlds.items()}
    for r, (_, pr) in worlds.items():   # the schedule from step 0, whatever warm-up and capture left
        pr.acc.zero_()
        pr.mask.fill_(1)
        pr.step.zero_()
    torch.cuda.synchronize()
    times = {r: {"all": [], "acc": [], "pruned": []} for r in worlds}
    ncirc = {r: {"all": [], "pruned": []} for r in worlds}
    for _ in range(rounds):
        for r, (_, pr) in worlds.items():
            per = {"acc": [], "pruned": []}
            for _s in range(3 * periods):
                kind = "acc" if int(pr.step) % 3 == 0 else "pruned"
                c = circuits(pr.mask)
                per[kind].append(timed(graphs[r].replay, 1))
                ncirc[r]["all"].append(c)
                if kind == "pruned":
                    ncirc[r]["pruned"].append(c)
            times[r]["all"].append(statistics.mean(per["acc"] + per["pruned"]))
            times[r]["acc"].append(statistics.median(per["acc"]))
            times[r]["pruned"].append(statistics.median(per["pruned"]))
    for r in worlds:
        t = times[r]
        lines.append(f"{r:>6}  {cell(t['all'], 9, 3):>30}  {cell(t['acc'], 9, 3):>30}  {cell(t['pruned'], 9, 3):>30}  "
                     f"{statistics.mean(ncirc[r]['all']):>13.1f}  {statistics.mean(ncirc[r]['pruned']):>24.1f}")
        print(lines[-1], flush=True)
    t0, t5 = statistics.median(times[0.0]["all"]), statistics.median(times[0.5]["all"])
    c0, c5 = statistics.mean(ncirc[0.0]["all"]), statistics.mean(ncirc[0.5]["all"])
    lines.append(f"ratio 0.5 / ratio 0: time {t5 / t0:.3f}, circuits {c5 / c0:.3f}; pruned steps alone: time "
                 f"{statistics.median(times[0.5]['pruned']) / statistics.median(times[0.0]['pruned']):.3f}, circuits "
                 f"{statistics.mean(ncirc[0.5]['pruned']) / statistics.mean(ncirc[0.0]['pruned']):.3f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--periods", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measured_step_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = ["The QSC training step under shots and device noise: python scripts/measured_step_timing.py",
             f"{torch.cuda.get_device_name(0)}; HIP events, median (min .. max) over {args.rounds} rounds, variants "
             f"alternating within a round; (a) {args.iters} steps per round and variant"]
    part_a(dev, args.rounds, args.iters, lines)
    part_b(dev, args.rounds, args.periods, lines)
    part_b(dev, args.rounds, args.periods, lines, streams=9)
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
