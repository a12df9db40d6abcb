"""Noise-aware adjoint gradients on the host: the ``cpu`` backend's G against a central finite difference of Ebar,
Ebar against its formula written out here and against the noisy shots forward's mean, the difference to the
straight-through gradient, the ``diff_method="noisy_adjoint"`` API and the runner's knobs."""
import functools
import math
import warnings

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128, QuantumLayer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (DIFF_METHODS, NoiseModel,
                                                                                         noise_sites,
                                                                                         noisy_adjoint_rows,
                                                                                         pauli_frames, qsim,
                                                                                         qsim_probs, z_signs)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner

SEED, CTR = 7, 3
RATES = (0.05, 0.1, 0.03, 0.05)
NOISE = NoiseModel(*RATES)
FD_TOL = 1e-4
SHAPES = [(3, 2, 3, 8), (4, 2, 3, 8)]


@functools.lru_cache(maxsize=None)
def inputs(n, L, B):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi
    gE = torch.randn(B, n, generator=torch.Generator().manual_seed(2))
    return x, w, gE


def ebar_formula(x, w, noise, T, seed=SEED, ctr=CTR):
    """Ebar[b, j] = c_j (1/T) sum_tau s_j(tau) E_j^tau + d_j in fp64, from the frames and the framed oracle."""
    B, n = x.shape
    L = w.shape[-3]
    F = pauli_frames(noise_sites(noise, B, n, L, T, seed, ctr))
    E = (qsim_probs(x.repeat_interleave(T, dim=0), w, "cpu", frames=F.view(B * T, L, 2))
         @ z_signs(n, dtype=torch.float64)).view(B, T, n)
    s = torch.empty(B, T, n, dtype=torch.float64)
    for j in range(n):
        s[:, :, j] = 1.0 - 2.0 * ((F[:, :, L - 1, 0] >> j) & 1).double()
    thr = torch.from_numpy(noise.thresholds_host(n)[2].astype("int64")).double()
    c = 1.0 - (thr[:, 0] + thr[:, 1]) / 65536.0
    d = (thr[:, 1] - thr[:, 0]) / 65536.0
    return c * (s * E).mean(1) + d


@functools.lru_cache(maxsize=None)
def rows(n, L, B, T):
    x, w, gE = inputs(n, L, B)
    return noisy_adjoint_rows(x, w, gE, NOISE, T, SEED, CTR, "cpu", return_expectation=True)


@pytest.mark.parametrize("n,L,B,T", SHAPES)
def test_definition_against_a_finite_difference(n, L, B, T):
    x, w, gE = inputs(n, L, B)
    G, Ebar = rows(n, L, B, T)
    assert G.shape == (B, 2 * n * L) and G.dtype == torch.float32 and Ebar.dtype == torch.float64
    want = ebar_formula(x, w, NOISE, T)
    e = float((Ebar - want).abs().max())
    print(f"|Ebar - formula| = {e:.2e}")
    assert e <= 1e-12
    # Central difference of the formula, h = 1e-3.  The oracle takes fp32 weights: the step is the difference of the
    # two fp32 weights actually passed, so their rounding does not enter the quotient.
    h, P = 1e-3, 2 * n * L
    fd = torch.empty(B, P, dtype=torch.float64)
    for p in range(P):
        wp, wm = w.clone(), w.clone()
        wp.view(-1)[p] += h
        wm.view(-1)[p] -= h
        step = float(wp.view(-1)[p].double() - wm.view(-1)[p].double())
        fd[:, p] = (gE.double() * (ebar_formula(x, wp, NOISE, T) - ebar_formula(x, wm, NOISE, T))).sum(1) / step
    e = float((G.double() - fd).abs().max())
    print(f"|G - finite difference| = {e:.2e} (tol {FD_TOL:.0e}), |G|max = {float(G.abs().max()):.3f}")
    assert e <= FD_TOL
    assert float(G.abs().max()) > 0.05


def test_ebar_is_the_mean_of_the_shots_forward():
    n, L, B, T = 4, 2, 3, 8
    shots = 1 << 18
    x, w, _ = inputs(n, L, B)
    Ebar = rows(n, L, B, T)[1]
    E = qsim(x, w, "cpu", shots=shots, seed=SEED, counter=CTR, noise=NOISE, trajectories=T).double()
    sigma = ((1.0 - Ebar ** 2) / shots).sqrt()
    z = (E - Ebar).abs() / sigma
    print(f"max |E - Ebar| / sigma = {float(z.max()):.2f}")
    assert bool((z <= 6.0).all())


def test_it_differs_from_the_straight_through_gradient():
    n, L, B, T = 4, 2, 3, 8
    x, w, gE = inputs(n, L, B)
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    (qsim(xa, wa, "cpu") * gE).sum().backward()
    G = rows(n, L, B, T)[0]
    diff = float((G.sum(0) - wa.grad.reshape(-1)).abs().max())
    print(f"|dw(noisy adjoint) - dw(noiseless adjoint)|max = {diff:.3f}")
    assert diff > 100 * FD_TOL
    # all rates zero: the noiseless adjoint
    G0, E0 = noisy_adjoint_rows(x, w, gE, NoiseModel(), T, SEED, CTR, "cpu", return_expectation=True)
    assert float((G0.sum(0) - wa.grad.reshape(-1)).abs().max()) <= 1e-6
    assert float((G0[:, 0:2 * n:2] - xa.grad).abs().max()) <= 1e-6
    assert float((E0 - qsim(x, w, "cpu").double()).abs().max()) <= 1e-6
    assert torch.equal(G0, noisy_adjoint_rows(x, w, gE, NoiseModel(), 1, SEED, CTR, "cpu"))


def test_autograd_is_the_rows():
    n, L, B, T, shots = 4, 2, 3, 8, 64
    x, w, gE = inputs(n, L, B)
    G = rows(n, L, B, T)[0]
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    kw = dict(shots=shots, seed=SEED, counter=CTR, noise=NOISE, trajectories=T)
    E = qsim(xa, wa, "cpu", diff_method="noisy_adjoint", **kw)
    assert torch.equal(E, qsim(x, w, "cpu", **kw))   # the forward is the noisy shots forward
    (E * gE).sum().backward()
    assert torch.equal(xa.grad, G[:, 0:2 * n:2]) and torch.equal(wa.grad.reshape(-1), G.sum(0))
    # grouped weights: group g's samples run under w[g]; the master gradient sits in group 0
    wg = torch.stack([w, w + 0.1, w - 0.2])
    Gg = noisy_adjoint_rows(x, wg, gE, NOISE, T, SEED, CTR, "cpu")
    wga = wg.clone().requires_grad_()
    (qsim(x, wga, "cpu", diff_method="noisy_adjoint", **kw) * gE).sum().backward()
    assert torch.equal(wga.grad[0].reshape(-1), Gg.sum(0)) and float(wga.grad[1:].abs().max()) == 0
    assert not torch.equal(Gg[1:], G[1:]) and torch.equal(Gg[:1], G[:1])


def test_range_checks():
    x, w, gE = inputs(4, 2, 3)
    assert "noisy_adjoint" in DIFF_METHODS
    with pytest.raises(ValueError, match="noise"):
        qsim(x, w, "cpu", shots=64, diff_method="noisy_adjoint")
    with pytest.raises(ValueError, match="shots"):
        qsim(x, w, "cpu", diff_method="noisy_adjoint")
    with pytest.raises(ValueError, match="shots"):
        qsim(x, w, "cpu", diff_method="noisy_adjoint", noise=NOISE)
    with pytest.raises(ValueError, match="shots"):   # the existing refusal stays
        qsim(x, w, "cpu", noise=NOISE)
    with pytest.raises(ValueError, match="shift_mask"):
        qsim(x, w, "cpu", shots=64, diff_method="noisy_adjoint", noise=NOISE,
             shift_mask=torch.ones(2, 4, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="torch"):
        qsim(x, w, "torch", shots=64, diff_method="noisy_adjoint", noise=NOISE)
    with pytest.raises(ValueError, match="multiple"):
        qsim(x, w, "cpu", shots=64, diff_method="noisy_adjoint", noise=NOISE, trajectories=3)
    with pytest.raises(ValueError, match="torch"):
        noisy_adjoint_rows(x, w, gE, NOISE, 4, backend="torch")
    for T in (0, 1025):
        with pytest.raises(ValueError, match="trajectories"):
            noisy_adjoint_rows(x, w, gE, NOISE, T, backend="cpu")
    with pytest.raises(ValueError, match="NoiseModel"):
        noisy_adjoint_rows(x, w, gE, None, 4, backend="cpu")
    with pytest.raises(ValueError, match="error sites"):
        noisy_adjoint_rows(torch.zeros(1, 2), torch.zeros(1025, 2, 2), torch.zeros(1, 2), NOISE, backend="cpu")
    with pytest.raises(NotImplementedError, match="12"):
        noisy_adjoint_rows(torch.zeros(1, 13), torch.zeros(1, 13, 2), torch.zeros(1, 13), NOISE, backend="cpu")
    # needs no shots: 3 trajectories are fine here
    assert noisy_adjoint_rows(x, w, gE, NOISE, 3, backend="cpu").shape == (3, 16)


def test_modules_pass_noisy_adjoint_through():
    n, L, B = 4, 2, 3
    x, _, gE = inputs(n, L, B)
    q = QuantumLayer(n, L, "cpu")
    q.shots, q.diff_method, q.noise, q.trajectories = 64, "noisy_adjoint", NOISE, 4   # plain attributes
    q.manual_shot_seed(SEED)
    (q(x) * gE).sum().backward()
    G = noisy_adjoint_rows(x, q.weights.detach(), gE, NOISE, 4, SEED, 0, "cpu")
    assert torch.equal(q.weights.grad.reshape(-1), G.sum(0))
    torch.manual_seed(0)
    m = QSC_P128(n_qubits=n, n_layers=L, backend="cpu", shots=64, diff_method="noisy_adjoint", noise=NOISE,
                 trajectories=4)
    assert m.qlayer.diff_method == "noisy_adjoint" and m.qlayer.noise is NOISE and m.qlayer.trajectories == 4
    torch.nn.functional.nll_loss(m.train()(torch.randn(B, 2, 16, 8)), torch.arange(B) % 3).backward()
    assert float(m.qlayer.weights.grad.abs().max()) > 0 and m.preprocess[0].weight.grad is not None


def test_runner_trains_noisy_adjoint(tmp_path):
    r = Y2HRunner(n_epochs=1, data_len=60, batch_size_DML=16, device="cpu", workspace=str(tmp_path / "a"),
                  data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2, use_quantumnat=True,
                  seed=0, qsc_diff_method="noisy_adjoint", qsc_shots=64, qsc_noise_p1=1e-3, qsc_noise_p2=1e-2,
                  qsc_readout01=0.02, qsc_readout10=0.02, qsc_trajectories=4)
    torch.manual_seed(0)
    w0 = QSC_P128(4, 2, 3).qlayer.weights.detach().clone()   # the runner seeds the same way before building
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (synthetic-data notice)
        m = r.train_QSC_P128()
    assert m.qlayer.diff_method == "noisy_adjoint" and m.qlayer.shots == 64 and m.qlayer.trajectories == 4
    assert isinstance(m.qlayer.noise, NoiseModel)
    assert len(r.train_QSC_losses) == 1 and all(math.isfinite(v) for v in r.train_QSC_losses)
    assert all(bool(torch.isfinite(v).all()) for v in m.state_dict().values())
    assert not torch.equal(m.qlayer.weights.detach().cpu(), w0)


def test_runner_refuses_noisy_adjoint_without_rates_or_shots(tmp_path):
    for knobs in (dict(qsc_shots=64), dict(qsc_noise_p1=1e-3), {}):
        r = Y2HRunner(device="cpu", workspace=str(tmp_path / "w"), data_dir=str(tmp_path / "data"),
                      qsc_diff_method="noisy_adjoint", **knobs)
        with pytest.raises(ValueError, match="qsc_shots"):
            r.train_QSC_P128()
