"""Time the streamed finite-shot path (csrc/hip/qsim_stream.hip's probabilities pass, csrc/hip/qsim_stream_shots.hip)
against the exact streamed forward, at n = 13..16.

For every configuration (B, n, L, shots) the variants run on the same inputs:
  fused      qd_qsim_stream_shots_fwd (forward passes, probabilities pass with run totals, block sampler, counts)
  two-stage  qd_qsim_stream_probs then qd_stream_sample_z (run totals recomputed from the probabilities)
  exact      the exact <Z> forward, qd_qsim_stream_fwd
  probs, sample_z   the two stages on their own (which launch a difference sits in)
The protocol is scripts/shots_timing.py's: each variant is captured once as a HIP graph of ITERS back-to-back calls,
warmed up and replayed between two events; the variants alternate within a round and the table gives the median and
the min .. max over the rounds, per call.  The fused and two-stage outputs are compared bit for bit first.  Every
qubit count runs in a child process of its own under a time limit; a child that fails ends the run.

    python scripts/shots_stream_timing.py [--qubits 13 14 16] [--rounds 5] [--iters 20] [--out FILE]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, L, SHOTS, SEED = 2304, 3, 1024, 1234
HEAD = (f"{'B':>5} {'n':>3} {'L':>2} {'shots':>6}  {'fused':>24}  {'two-stage':>24}  {'exact fwd':>24}  {'probs':>24}  "
        f"{'sample_z':>24}  fused/exact  fused-exact  max|E_shots-E_exact|")


def one(n: int, rounds: int, iters: int) -> str:
    import torch
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import cell, time_graphed
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x = (torch.rand(B, n) * 2 - 1).to(dev)
    w = (torch.rand(L, n, 2) * 2 * math.pi).to(dev)
    E, E2, Ex, E3 = (torch.empty(B, n, device=dev) for _ in range(4))
    probs = torch.empty(B, 1 << n, device=dev)
    probs2 = torch.empty(B, 1 << n, device=dev)

    def fused():
        Q.hip_qsim_shots_fwd(x, w, E, None, SHOTS, SEED)

    def two_stage():
        Q.hip_qsim_probs(x, w, probs)
        Q.hip_sample_z(probs, E2, None, n, SHOTS, SEED)

    def exact():
        Q.hip_qsim_fwd(x, w, Ex)

    def probs_only():
        Q.hip_qsim_probs(x, w, probs2)

    def sample_only():
        Q.hip_sample_z(probs, E3, None, n, SHOTS, SEED)

    for f in (fused, two_stage, exact, probs_only, sample_only):
        f()
    torch.cuda.synchronize()
    assert torch.equal(E, E2) and torch.equal(E, E3), "fused and two-stage results differ"
    dE = float((E - Ex).abs().max())
    times = time_graphed({"fused": fused, "two-stage": two_stage, "exact": exact, "probs": probs_only,
                          "sample_z": sample_only}, iters, rounds)
    c = {k: cell(v, 8) for k, v in times.items()}
    mf, me = statistics.median(times["fused"]), statistics.median(times["exact"])
    return (f"{B:>5} {n:>3} {L:>2} {SHOTS:>6}  {c['fused']:>24}  {c['two-stage']:>24}  {c['exact']:>24}  {c['probs']:>24}  "
            f"{c['sample_z']:>24}  {mf / me:>11.2f}  {mf - me:>11.1f}  {dE:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[13, 14, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per qubit count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help="(internal) time this qubit count in this process")
    args = ap.parse_args()
    if args.one:
        print("ROW " + one(args.one, args.rounds, args.iters), flush=True)
        return
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import write_report
    lines = [f"per-call time in microseconds, median (min .. max) over {args.rounds} rounds of {args.iters} "
             f"graph-replayed calls, variants alternating within a round", HEAD]
    for n in args.qubits:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--rounds", str(args.rounds),
                            "--iters", str(args.iters)], capture_output=True, text=True, timeout=args.limit)
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            sys.exit(f"n={n}: exit status {r.returncode}\n{r.stdout}\n{r.stderr}")
        lines += rows
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
