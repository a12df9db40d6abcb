"""A demonstration, not a claim: does QuantumNAT post-measurement normalization / quantization help the 8-qubit QSC
survive a noisy device?

The README's shots demonstration (8 qubits, 12 epochs, 6000 synthetic samples per stream, 10 dB) is trained three
ways with the runner -- without post-processing, with normalization, with normalization + 5 levels (penalty weight
0.1) -- in simulation (exact expectations, QuantumNAT weight noise on), and each model classifies 6000 fresh 10 dB
test samples three ways through the HIP inference kernels (QSCStepHIP.infer, chunks of 2304): exact; at the README's
noise point (p1 = 1e-3, p2 = 1e-2, readout 0.02 / 0.02, T = 64, 1024 shots); at ten times those rates.  Models with
post-processing normalize each chunk with its own statistics (qsc_post_stats = batch; the running statistics'
accuracy is printed beside it).

    python scripts/postmeas_eval.py [--epochs 12] [--data-len 6000] [--seed 1234] [--out profiles/postmeas_eval.txt]
"""
import argparse
import os
import sys
import tempfile
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.data.channel import generate_mixed, pack_pilots  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import NoiseModel  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner  # noqa: E402

TRAIN = {"plain": {}, "norm": dict(qsc_post_norm=True),
         "norm + 5 levels": dict(qsc_post_norm=True, qsc_post_quant_levels=5, qsc_post_quant_weight=0.1)}
DEVICES = {"exact": None, "noise point": (1e-3, 1e-2, 0.02, 0.02), "10 x noise point": (1e-2, 1e-1, 0.2, 0.2)}
CHUNK, SHOTS, T = 2304, 1024, 64


@torch.no_grad()
def accuracy(model, x, ind, rates, seed, stats):
    dev = x.device
    model = model.to(dev).eval()
    if getattr(model, "postmeas", None) is not None:
        model.postmeas.stats = stats
    step = QSCStepHIP(model, FlatParamSpace(list(model.named_parameters()), dev), CHUNK)
    xin = torch.empty((CHUNK,) + tuple(x.shape[1:]), device=dev)
    pred = torch.empty(CHUNK, dtype=torch.int64, device=dev)
    out = torch.empty(x.shape[0], dtype=torch.int64, device=dev)
    noise = NoiseModel(*rates) if rates else None
    for lo in range(0, x.shape[0], CHUNK):
        n = min(CHUNK, x.shape[0] - lo)
        xin[:n].copy_(x[lo:lo + n])
        if n < CHUNK:
            xin[n:].copy_(x[lo + n - 1:lo + n].expand(CHUNK - n, *x.shape[1:]))
        if rates:
            step.infer(xin, pred, shots=SHOTS, seed=seed, counter=lo // CHUNK, noise=noise, trajectories=T, valid=n)
        else:
            step.infer(xin, pred, valid=n)
        out[lo:lo + n].copy_(pred[:n])
    return float((out == ind).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--data-len", type=int, default=6000)
    ap.add_argument("--test-len", type=int, default=6000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postmeas_eval.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = ["QuantumNAT post-measurement processing, a demonstration: python scripts/postmeas_eval.py",
             f"{torch.cuda.get_device_name(0)}; 8-qubit QSC, {args.epochs} epochs, {args.data_len} synthetic samples per "
             f"stream, 10 dB, seed {args.seed}; accuracy on {args.test_len} test samples, chunks of {CHUNK}; noisy "
             f"devices: {SHOTS} shots over T = {T}",
             f"{'trained':>16}  {'val acc':>8}  " + "  ".join(f"{k:>24}" for k in DEVICES)
             + "   (batch statistics / running statistics)"]
    Yp, _, _, ind = generate_mixed(args.test_len, 10.0, 128, -1, base_seed=args.seed,
                                   split=f"test@{args.data_len * 3}", device=dev)
    x = pack_pilots(Yp, 128).contiguous().float()
    with tempfile.TemporaryDirectory() as tmp:
        for name, knobs in TRAIN.items():
            r = Y2HRunner(n_epochs=args.epochs, data_len=args.data_len, device="cuda", SNRdb=10, n_qubits=8,
                          workspace=os.path.join(tmp, name.replace(" ", "_")), data_dir=os.path.join(tmp, "data"),
                          print_freq=100000, seed=args.seed, **knobs)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = r.train_QSC_P128()
            cells = []
            for dname, rates in DEVICES.items():
                a = accuracy(m, x, ind, rates, args.seed, "batch")
                if knobs:
                    cells.append(f"{a:.4f} / {accuracy(m, x, ind, rates, args.seed, 'running'):.4f}")
                else:
                    cells.append(f"{a:.4f}")
            lines.append(f"{name:>16}  {max(r.val_QSC_accuracies):8.4f}  " + "  ".join(f"{c:>24}" for c in cells))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
