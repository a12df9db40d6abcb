"""The ``hip`` leg of tests/test_qsim_refusals_cpu.py: the same table on CUDA tensors at (n, L) = (2, 1), every row
with ``shots`` set again at n = 13 (past the measured kernels' 12 qubits: refused before any launch), and the
tensor ``counter``s that are refused, against tests/golden/qsim_refusals_hip.json -- recorded, like the host file,
at the commit before the resolver (run this file as a script on a GPU to record it again)."""
import sys

import pytest
import torch

from test_qsim_refusals_cpu import key, load, mismatches, outcome, save, table

pytestmark = pytest.mark.gpu

GOLDEN = "qsim_refusals_hip.json"
# (diff_method, shots, noise): one accepted call of every measured mode, for the counters
MODES = (("adjoint", 8, "none"), ("adjoint", 8, "model"), ("parameter_shift", None, "none"),
         ("parameter_shift", 8, "none"), ("on_chip", 8, "model"), ("noisy_adjoint", 8, "model"))
COUNTERS = {"int32": lambda: torch.zeros((), dtype=torch.int32, device="cuda"),
            "host": lambda: torch.zeros((), dtype=torch.int64),
            "numel2": lambda: torch.zeros(2, dtype=torch.int64, device="cuda")}


def run_all():
    got = {key(c): outcome(c, "cuda") for c in table(("hip",), ((2, 1),))}
    got.update({key(c): outcome(c, "cuda") for c in table(("hip",), ((13, 1),), (8, 12))})
    for dm, shots, noise in MODES:
        for name, make in COUNTERS.items():
            case = ("hip", dm, shots, noise, 1, "none", (2, 1))
            got[key(case) + "|counter=" + name] = outcome(case, "cuda", counter=make())
    return got


def test_every_case_of_the_hip_grid_ends_as_recorded(cuda):
    want = load(GOLDEN)
    got = run_all()
    bad = mismatches(got, want)
    assert not bad, f"{len(bad)} of {len(got)} cases differ:\n" + "\n".join(bad[:40])
    for k, o in got.items():
        if k.endswith("|13,1") and got[k.replace("|13,1", "|2,1")] == "ok":   # a legal mode, too many qubits
            assert o[0] == "NotImplementedError", (k, o)
        if "|counter=" in k:
            assert o != "ok" and o[0] == "ValueError", (k, o)


if __name__ == "__main__":
    rec = run_all()
    save(GOLDEN, rec)
    print(len(rec), "cases,", sum(o == "ok" for o in rec.values()), "ok", file=sys.stderr)
