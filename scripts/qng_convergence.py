"""A demonstration, not a claim: the 8-qubit QSC trained with and without the quantum natural gradient.

The README's QSC demonstration (8 qubits, 3 layers, synthetic samples per stream at 10 dB, QuantumNAT weight noise on)
is trained with the runner's exact fused step three ways -- AdamW on the raw gradient, and on the natural gradient
with lam = 0.01 and 0.1 -- for every seed, and the per-epoch training loss and validation accuracy are written out.

    python scripts/qng_convergence.py [--epochs 8] [--data-len 6000] [--seeds 1234,77] [--out reports/qng_convergence.md]
"""
import argparse
import os
import sys
import tempfile
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner  # noqa: E402

TRAIN = {"AdamW": {}, "QNG lam=0.01": dict(qsc_qng=True, qsc_qng_lambda=0.01),
         "QNG lam=0.1": dict(qsc_qng=True, qsc_qng_lambda=0.1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--data-len", type=int, default=6000)
    ap.add_argument("--seeds", default="1234,77")
    ap.add_argument("--out", default=os.path.join(ROOT, "reports", "qng_convergence.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    seeds = [int(s) for s in args.seeds.split(",")]
    lines = ["# QSC training with and without the quantum natural gradient", "",
             "A demonstration, not a claim: `python scripts/qng_convergence.py`.  " + torch.cuda.get_device_name(0)
             + f"; 8-qubit, 3-layer QSC, {args.epochs} epochs, {args.data_len} synthetic samples per stream, 10 dB, "
             "QuantumNAT weight noise on, the exact fused step; validation accuracy after every epoch, then the last "
             "epoch's training loss.", "",
             "| seed | optimizer | " + " | ".join(f"epoch {e + 1}" for e in range(args.epochs)) + " | final train loss |",
             "|---|---|" + "---|" * (args.epochs + 1)]
    with tempfile.TemporaryDirectory() as tmp:
        for seed in seeds:
            for name, knobs in TRAIN.items():
                r = Y2HRunner(n_epochs=args.epochs, data_len=args.data_len, device="cuda", SNRdb=10, n_qubits=8,
                              workspace=os.path.join(tmp, f"{seed}_{name.replace(' ', '_')}"),
                              data_dir=os.path.join(tmp, "data"), print_freq=100000, seed=seed, **knobs)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    r.train_QSC_P128()
                lines.append(f"| {seed} | {name} | " + " | ".join(f"{a:.4f}" for a in r.val_QSC_accuracies)
                             + f" | {r.train_QSC_losses[-1]:.4f} |")
                print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
