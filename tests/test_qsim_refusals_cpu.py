"""Which argument combinations ``qsim`` accepts, and how it refuses the others: the Cartesian product of backend,
``diff_method``, ``shots``, ``noise``, ``trajectories``, ``shift_mask`` and (n, L), every case run forward and
backward, against the outcomes recorded in tests/golden/qsim_refusals.json ("ok", or the exception's type and full
message).  The file was recorded at the commit before the measurement arguments got their one resolver, so it pins
the order in which the refusals fire; record it again (run this file as a script) only when a refusal changes on
purpose."""
import itertools
import json
import os
import sys

import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import MAX_SHOTS, NoiseModel, qsim

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 2
BACKENDS = ("cpu", "torch", "cuda")                       # "cuda" is no backend's name
METHODS = ("adjoint", "parameter_shift", "on_chip", "noisy_adjoint", "finite_diff")
SHOTS = (None, 0, 8, 12, MAX_SHOTS + 1)
NOISES = ("none", "model", "float")
TRAJECTORIES = (1, 2, 3)
MASKS = ("none", "right", "wrong")
SHAPES = ((2, 1), (2, 2))
MODEL = NoiseModel(0.05, 0.1, 0.03, 0.05)


def table(backends=BACKENDS, shapes=SHAPES, shots=SHOTS):
    return list(itertools.product(backends, METHODS, shots, NOISES, TRAJECTORIES, MASKS, shapes))


def key(case) -> str:
    be, dm, shots, noise, T, mask, (n, L) = case
    return f"{be}|{dm}|{shots}|{noise}|{T}|{mask}|{n},{L}"


def outcome(case, device="cpu", **extra):
    """"ok", or [exception type, message], of qsim(...).sum().backward() for one row of the table."""
    be, dm, shots, noise, T, mask, (n, L) = case
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, n, generator=g) * 2 - 1).to(device).requires_grad_()
    w = (torch.rand(L, n, 2, generator=g) * 6.0).to(device).requires_grad_()
    shift_mask = {"none": None, "right": torch.ones(L, n, 2, dtype=torch.bool),
                  "wrong": torch.ones(L + 1, n, 2, dtype=torch.bool)}[mask]
    try:
        E = qsim(x, w, be, shots=shots, seed=5, diff_method=dm, shift_mask=shift_mask,
                 noise={"none": None, "model": MODEL, "float": 0.1}[noise], trajectories=T, **extra)
        E.sum().backward()
        assert E.shape == (B, n) and x.grad.shape == x.shape and w.grad.shape == w.shape
    except Exception as e:   # noqa: BLE001  (the outcome is the exception)
        return [type(e).__name__, str(e)]
    return "ok"


def load(name):
    """{case key: outcome} of a golden file: its outcomes are stored once and referred to by index."""
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        doc = json.load(f)
    return {k: doc["outcomes"][i] for k, i in doc["cases"].items()}


def save(name, got) -> None:
    outcomes = []
    for o in got.values():
        if o not in outcomes:
            outcomes.append(o)
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    with open(os.path.join(GOLDEN_DIR, name), "w") as f:
        json.dump({"outcomes": outcomes, "cases": {k: outcomes.index(o) for k, o in got.items()}}, f, indent=0)
        f.write("\n")


def mismatches(got, want):
    assert got.keys() == want.keys(), sorted(got.keys() ^ want.keys())[:10]
    return [f"{k}: got {got[k]!r}, recorded {want[k]!r}" for k in got if got[k] != want[k]]


def test_every_case_of_the_grid_ends_as_recorded():
    want = load("qsim_refusals.json")
    got = {key(c): outcome(c) for c in table()}
    assert len(got) == 4050
    bad = mismatches(got, want)
    assert not bad, f"{len(bad)} of {len(got)} cases differ:\n" + "\n".join(bad[:40])
    assert sum(o == "ok" for o in got.values()) == 68
    assert len({tuple(o) for o in got.values() if o != "ok"}) == 17


if __name__ == "__main__":
    rec = {key(c): outcome(c) for c in table()}
    save("qsim_refusals.json", rec)
    print(len(rec), "cases,", sum(o == "ok" for o in rec.values()), "ok,",
          len({tuple(o) for o in rec.values() if o != "ok"}), "distinct refusals", file=sys.stderr)
