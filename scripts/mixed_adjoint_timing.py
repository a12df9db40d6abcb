"""Time the density-matrix adjoint (csrc/hip/qsim_mixed.hip qd_qsim_mixed_adjoint) against the gradient it replaces.

For every configuration (B, n, L) four variants run on the same inputs, at the README's noise point:
  rows      ``mixed_adjoint_rows``, the public function, eager: its checks, G and the workspace allocated per call
  shift     ``mixed_rows``, the public function, eager: the +-pi/2 shift rule, 2 . 2nL forwards over the shifted weights
  adjoint   the raw launcher ``hip_qsim_mixed_adjoint`` alone, G and the workspace preallocated, graph-replayed
  forward   one ``qd_qsim_mixed_fwd``, graph-replayed, for scale
(shift / rows compares like with like, two eager functions; adjoint / forward two kernels.)
and, last, one fused ``qsc_noise_exact`` training step (ops/qsc.py QSCStepHIP(exact_noise=True)) at 9 x 256 samples
with three QuantumNAT streams.  The kernels and the step are captured once as a HIP graph of ITERS back-to-back
repetitions and replayed between two events; the two public functions run ITERS eager repetitions between the events
instead.  The variants alternate within a
round, after two warm-up calls each, and the table gives the median and the min .. max over the rounds, per repetition.

    python scripts/mixed_adjoint_timing.py [--rounds 5] [--iters 3] [--out profiles/mixed_adjoint_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import (alternate, cell, graph_of,  # noqa: E402
                                                                                             time_graphed, write_report)

CONFIGS = [(256, 4, 3), (256, 6, 3), (256, 7, 3), (256, 8, 3)]
NOISE = Q.NoiseModel(1e-3, 1e-2, 0.02, 0.02)
STEP = (9 * 256, 8, 3, 3)   # samples, n, L, QuantumNAT streams


def variants(B, n, L, dev):
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    gE = (torch.rand(B, n) * 2 - 1).to(dev)
    G, E = torch.empty(B, 2 * n * L, device=dev), torch.empty(B, n, device=dev)
    ws = Q.mixed_adjoint_workspace(n, B, dev)
    out = {}

    def adjoint():
        Q.hip_qsim_mixed_adjoint(x, w, gE, G, None, NOISE, 0, ws)

    def rows():
        out["rows"] = Q.mixed_adjoint_rows(x, w, gE, NOISE)

    def shift():
        out["shift"] = Q.mixed_rows(x, w, gE, NOISE)

    def forward():
        Q.hip_qsim_mixed_fwd(x, w, E, None, NOISE, 0, ws)

    adjoint()
    rows()
    shift()
    forward()
    torch.cuda.synchronize()
    assert torch.equal(out["rows"], G)   # the public function is that launch
    err = float((G - out["shift"]).abs().max())   # two fp32 evaluations of one gradient
    assert math.isfinite(err) and err <= 1e-3, err
    return {"rows": rows, "shift": shift, "adjoint": adjoint, "forward": forward}, err


def fused_step(dev):
    B, n, L, S = STEP
    torch.manual_seed(0)
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=True, use_gradient_pruning=False, pilot_num=128).to(dev).train()
    space = FlatParamSpace(list(m.named_parameters()), dev)
    step = QSCStepHIP(m, space, B, n_groups=S, noise=NOISE, exact_noise=True)
    x = torch.randn(B, 2, 16, 8, device=dev)
    y = torch.randint(0, 3, (B,), device=dev)

    def run():
        step(x, y, accumulate=False)

    run()
    torch.cuda.synchronize()
    assert math.isfinite(float(step.loss))
    return {"step": run}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_adjoint_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = ["Density-matrix adjoint (csrc/hip/qsim_mixed.hip qd_qsim_mixed_adjoint) against the shift rule over forward "
             "launches (mixed_rows) and one forward; rows / shift: the public functions, eager; adjoint / forward: "
             "the raw launchers, graph-replayed; noise 1e-3 / 1e-2 / readout .02: python "
             "scripts/mixed_adjoint_timing.py",
             f"{torch.cuda.get_device_name(0)}; time per gradient / forward in microseconds, median (min .. max) over "
             f"{args.rounds} rounds of {args.iters} repetitions, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2}  {'mixed_adjoint_rows (eager)':>30}  {'mixed_rows (eager, 4nL forwards)':>34}  "
             f"{'raw adjoint launch':>30}  {'one forward':>28}  shift/rows  ranges apart  adjoint/forward  "
             f"max|G_adjoint-G_shift|"]
    for B, n, L in CONFIGS:
        fns, err = variants(B, n, L, dev)
        graphs = {k: graph_of(fns[k], args.iters) for k in ("adjoint", "forward")}

        def eager(f):
            def run():
                for _ in range(args.iters):
                    f()
            return run

        times = alternate({"rows": eager(fns["rows"]), "shift": eager(fns["shift"]),
                           "adjoint": graphs["adjoint"].replay, "forward": graphs["forward"].replay},
                          args.rounds, 1, 1e3 / args.iters)
        cells = {k: cell(v, 9) for k, v in times.items()}
        med = {k: statistics.median(v) for k, v in times.items()}
        apart = "yes" if max(times["rows"]) < min(times["shift"]) or min(times["rows"]) > max(times["shift"]) else "NO"
        lines.append(f"{B:>5} {n:>3} {L:>2}  {cells['rows']:>30}  {cells['shift']:>34}  {cells['adjoint']:>30}  "
                     f"{cells['forward']:>28}  {med['shift'] / med['rows']:>10.1f}  {apart:>12}  "
                     f"{med['adjoint'] / med['forward']:>15.2f}  {err:>22.3e}")
        print(lines[-1], flush=True)
    B, n, L, S = STEP
    times = time_graphed(fused_step(dev), args.iters, args.rounds)
    lines.append(f"fused qsc_noise_exact step (preprocess, density-matrix forward, head, adjoint, preprocess backward; "
                 f"{B} samples, n = {n}, L = {L}, {S} QuantumNAT streams): {cell(times['step'], 9).strip()}")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
