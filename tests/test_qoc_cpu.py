"""QOC probabilistic gradient pruning on the host: the C++ twin of csrc/hip/qoc.hip's update (the schedule, the
mask's size, the sampling weights and their frequencies), the mask as ``pshift_rows``' ``shift_mask``, and the
runner's qsc_prune_* knobs on the ``cpu`` backend (masked parameters get no gradient; the resume file carries the
pruner)."""
import math
import warnings

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qoc import QOCPruner
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import pshift_rows
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train import checkpoint as ck
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner

SEED = 20240607   # (fixed before any draw was looked at)


def grads(P, steps, seed=1):
    g = torch.randn(steps, P, generator=torch.Generator().manual_seed(seed))
    g[:, 0] = 0.0
    g[1, P - 1] = float("nan")
    return g


@pytest.mark.parametrize("wa,wp", [(1, 2), (2, 3)])
@pytest.mark.parametrize("P,ratio", [(6, 0.5), (48, 0.5), (72, 0.9), (500, 0.25)])
def test_schedule_and_mask_size(P, ratio, wa, wp):
    pr = QOCPruner(P, ratio, wa, wp, SEED)
    K = P - math.floor(ratio * P)
    assert pr.K == K and bool(pr.mask.all()) and int(pr.step) == 0
    for s, g in enumerate(grads(P, 3 * (wa + wp))):
        acc0 = pr.acc.clone()
        pr.update(g)
        assert int(pr.step) == s + 1
        t, t1 = s % (wa + wp), (s + 1) % (wa + wp)
        want = torch.zeros(P) if t == 0 else acc0.clone()
        if t < wa:
            want = want + torch.where(torch.isfinite(g), g.abs(), torch.zeros(()))
        assert torch.equal(pr.acc, want), s
        assert set(pr.mask.tolist()) <= {0, 1}
        assert int(pr.mask.sum()) == (P if t1 < wa else K), s


def test_ratio_zero_is_no_mask():
    n, L, B = 3, 2, 4
    P = 2 * n * L
    pr = QOCPruner(P, 0.0, 1, 2, SEED)
    torch.manual_seed(0)
    x, w, gE = torch.rand(B, n) * 2 - 1, torch.rand(L, n, 2) * 6, torch.randn(B, n)
    plain = pshift_rows(x, w, gE, "cpu", shots=32, seed=3, counter=5)
    for g in grads(P, 6):
        pr.update(g)
        assert bool(pr.mask.all())
        assert torch.equal(pshift_rows(x, w, gE, "cpu", shots=32, seed=3, counter=5,
                                       shift_mask=pr.mask.view(L, n, 2)), plain)


def test_mask_prunes_the_rows():
    n, L, B = 3, 2, 4
    P = 2 * n * L
    pr = QOCPruner(P, 0.5, 1, 2, SEED)
    pr.update(torch.randn(P, generator=torch.Generator().manual_seed(4)))
    assert int(pr.mask.sum()) == P // 2
    torch.manual_seed(0)
    x, w, gE = torch.rand(B, n) * 2 - 1, torch.rand(L, n, 2) * 6, torch.randn(B, n)
    full = pshift_rows(x, w, gE, "cpu", shots=32, seed=3, counter=5)
    G = pshift_rows(x, w, gE, "cpu", shots=32, seed=3, counter=5, shift_mask=pr.mask.view(L, n, 2), need_dx=False)
    keep = pr.mask.bool()
    assert torch.equal(G[:, keep], full[:, keep]) and not bool(G[:, ~keep].any())


def test_all_zero_accumulator_is_uniform():
    """No gradient seen (acc = 0): every weight is 1, so a draw is u P >> 32 -- every parameter comes up, evenly."""
    P, N = 4, 2048
    pr = QOCPruner(P, 0.75, 1, 1, SEED)
    counts = torch.zeros(P)
    for _ in range(N):
        pr.update(torch.zeros(P))   # accumulation steps add 0; every second update draws
        if int(pr.step) % 2 == 1:
            assert int(pr.mask.sum()) == 1
            counts += pr.mask
    n = N // 2
    assert float((counts - n / P).abs().max()) <= 5 * math.sqrt(n * 0.25 * 0.75), counts


def test_draw_frequencies():
    """K = 1, acc = [1, 1, 2, 4]: q = [262145, 262145, 524289, 1048577], S = 2097156; 4096 draws over successive
    steps, every count within 5 sigma of N q_p / S."""
    acc = torch.tensor([1.0, 1.0, 2.0, 4.0])
    q = torch.tensor([262145, 262145, 524289, 1048577], dtype=torch.float64)
    assert int(q.sum()) == 2097156
    N = 4096
    pr = QOCPruner(4, 0.75, 1, 1, SEED)
    assert pr.K == 1
    counts = torch.zeros(4, dtype=torch.float64)
    for _ in range(N):
        pr.update(acc)            # step even: acc = |grad| = [1, 1, 2, 4], then the draw for the odd step
        assert torch.equal(pr.acc, acc) and int(pr.mask.sum()) == 1
        counts += pr.mask
        pr.update(torch.zeros(4))  # step odd: a pruning step; the next one accumulates again (all ones)
        assert bool(pr.mask.all())
    p = q / q.sum()
    bound = 5 * torch.sqrt(N * p * (1 - p))
    print("counts", counts.tolist(), "expected", (N * p).tolist(), "bound", bound.tolist())
    assert bool(((counts - N * p).abs() <= bound).all())


def test_value_errors():
    for kw in (dict(n_params=1, ratio=0.5), dict(n_params=4097, ratio=0.5), dict(n_params=8, ratio=1.0),
               dict(n_params=8, ratio=-0.1), dict(n_params=8, ratio=0.5, accum=0), dict(n_params=8, ratio=0.5, window=0)):
        with pytest.raises(ValueError):
            QOCPruner(**kw)
    with pytest.raises(ValueError, match="fp32"):
        QOCPruner(8, 0.5).update(torch.zeros(7))


# ------------------------------------------------------------------------------- the runner's knobs
def _runner(tmp_path, name, **knobs):
    return Y2HRunner(n_epochs=2, data_len=60, batch_size_DML=16, device="cpu", workspace=str(tmp_path / name),
                     data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=3, n_layers=2, use_quantumnat=True,
                     seed=0, **knobs)


def test_runner_trains_pruned(tmp_path, monkeypatch):
    seen = []
    update = QOCPruner.update

    def spy(self, grad):   # the mask the step ran under, and the raw gradient it left
        seen.append((self.mask.clone(), grad.detach().clone().reshape(-1), int(self.step)))
        update(self, grad)

    monkeypatch.setattr(QOCPruner, "update", spy)
    knobs = dict(qsc_diff_method="parameter_shift", qsc_shots=64, qsc_prune_ratio=0.5)
    r = _runner(tmp_path, "a", **knobs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = r.train_QSC_P128()
    assert len(r.train_QSC_losses) == 2 and all(math.isfinite(v) for v in r.train_QSC_losses)
    assert len(seen) >= 6
    pruned = 0
    for mask, grad, s in seen:
        assert int(mask.sum()) == (12 if s % 3 == 0 else 6), s
        assert not bool(grad[mask == 0].any()), s
        assert bool(grad[mask == 1].any()), s
        pruned += s % 3 != 0
    assert pruned >= 4
    assert m.qlayer.shift_mask is not None and tuple(m.qlayer.shift_mask.shape) == (2, 3, 2)
    # the resume file carries the pruner, and a resumed run restores it
    import glob
    files = glob.glob(str(tmp_path / "a" / "**" / "QSC_*_resume.pth"), recursive=True)
    assert len(files) == 1
    st = ck.load_resume(files[0])
    assert set(st["pruner"]) == {"acc", "mask", "step"} and int(st["pruner"]["step"]) == len(seen)
    restored = []
    load = QOCPruner.load_state_dict

    def spy_load(self, sd):
        load(self, sd)
        restored.append((self.acc.clone(), self.mask.clone(), int(self.step)))

    monkeypatch.setattr(QOCPruner, "load_state_dict", spy_load)
    r2 = _runner(tmp_path, "a", resume=True, **dict(knobs))
    r2.n_epochs = 3
    n_before = len(seen)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r2.train_QSC_P128()
    assert len(restored) == 1
    assert torch.equal(restored[0][0], st["pruner"]["acc"]) and torch.equal(restored[0][1], st["pruner"]["mask"])
    assert restored[0][2] == n_before and seen[n_before][2] == n_before   # the schedule goes on where it stopped


def test_runner_refuses_pruning_the_adjoint(tmp_path):
    for knobs in (dict(), dict(qsc_diff_method="noisy_adjoint", qsc_shots=64, qsc_noise_p1=1e-3)):
        r = _runner(tmp_path, "w", qsc_prune_ratio=0.5, **knobs)
        with pytest.raises(ValueError, match="qsc_prune_ratio"):
            r.train_QSC_P128()
    r = _runner(tmp_path, "w", qsc_step="graphed")
    with pytest.raises(ValueError, match="qsc_step"):
        r.train_QSC_P128()


def test_fused_step_falls_back_on_cpu(tmp_path):
    """qsc_step=fused on a CPU device is the module path: the same run as the default."""
    knobs = dict(qsc_diff_method="parameter_shift", qsc_shots=64)
    out = []
    for name, extra in (("m", {}), ("f", {"qsc_step": "fused"})):
        r = _runner(tmp_path, name, **knobs, **extra)
        r.n_epochs = 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = r.train_QSC_P128()
        out.append((r.train_QSC_losses, [v.clone() for v in m.state_dict().values()]))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
