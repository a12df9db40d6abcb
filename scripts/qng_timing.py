"""Time the quantum-natural-gradient launches (csrc/hip/qsim_metric.hip) against the circuit work a training step
already pays.

For every configuration (B, n, L) these variants run on the same inputs:
  metric    qd_qsim_metric: every sample's 2L metric blocks
  no-cov    qd_qsim_metric_nocov: the same launch without the covariance products on the matrix cores (its rows are
            not the metric) -- what the walk, the basis changes and the probabilities cost on their own
  reduce    qd_reduce_slab over the (B, 2L n n) rows
  solve     qd_qng_solve: 2L Cholesky solves
  qng       the three together, as QNGPreconditioner.precondition queues them
  fwd+adj   the exact forward and adjoint backward of qsim at the same shape (qsim.hip for n <= 10, qsim_big.hip
            above) with the slab reduction: the circuit cost of a step without the natural gradient
Each variant is captured once as a HIP graph of ITERS back-to-back repetitions (so the host's launch rate is not what
is timed), warmed up, and replayed between two events; the variants alternate within a round and the table gives the
median and the min .. max over the rounds, per repetition.

    python scripts/qng_timing.py [--rounds 5] [--iters 20] [--out profiles/qng_timing.txt]
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import qng as QN  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed, write_report  # noqa: E402

CONFIGS = [(2304, 8, 3), (256, 8, 3), (2304, 12, 3), (256, 12, 3)]
LAM = 0.01
_p, _i = ctypes.c_void_p, ctypes.c_int


def variants(B, n, L, dev):
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    gE = (torch.rand(B, n) * 2 - 1).to(dev)
    grad = torch.randn(L, n, 2).to(dev)
    work = grad.clone()
    rows = torch.empty(B, 2 * L * n * n, device=dev)
    rows_nc = torch.empty_like(rows)
    gsum = torch.empty(2 * L * n * n, device=dev)
    E = torch.empty(B, n, device=dev)
    dx = torch.empty(B, n, device=dev)
    dw = torch.empty(2 * n * L, device=dev)
    nocov_fn = nat.fn(nat.hip_lib(), "qd_qsim_metric_nocov", [_p, _p, _p, _i, _i, _i, _p])

    def metric():
        QN.hip_metric_rows(x, w, rows)

    def nocov():
        nat.check(nocov_fn(nat.ptr(x), nat.ptr(w), nat.ptr(rows_nc), B, n, L, nat.stream_ptr(dev)), "nocov")

    def reduce():
        Q.reduce_slab(rows, gsum)

    def solve():
        work.copy_(grad)
        QN.hip_qng_solve(gsum, B, LAM, work)

    def qng():
        metric()
        reduce()
        solve()

    def fwd_adj():
        Q.hip_qsim_fwd(x, w, E)
        Q.reduce_slab(Q.hip_qsim_bwd_slab(x, w, gE, dx), dw)

    fns = {"metric": metric, "no-cov": nocov, "reduce": reduce, "solve": solve, "qng": qng, "fwd+adj": fwd_adj}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qng_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    names = ["metric", "no-cov", "reduce", "solve", "qng", "fwd+adj"]
    lines = [f"{torch.cuda.get_device_name(0)}; time per repetition in microseconds, median (min .. max) over "
             f"{args.rounds} rounds of {args.iters} graph-replayed repetitions, variants alternating within a round",
             f"{'B':>5} {'n':>3} {'L':>2}  " + "  ".join(f"{k:>26}" for k in names)
             + "  qng/(fwd+adj)  cov share of metric"]
    for B, n, L in CONFIGS:
        times = time_graphed(variants(B, n, L, dev), args.iters, args.rounds)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"{B:>5} {n:>3} {L:>2}  " + "  ".join(f"{cell(times[k], 8):>26}" for k in names)
                     + f"  {med['qng'] / med['fwd+adj']:>13.2f}  {1 - med['no-cov'] / med['metric']:>19.2f}")
    lines.append("cov share = 1 - no-cov / metric: the part of the metric launch that the covariance products on the "
                 "matrix cores account for (solve includes the copy that restores its right-hand side)")
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
