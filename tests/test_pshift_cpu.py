"""Parameter-shift gradients of the QSC circuit on the host (ops/quantum.py, composed from the C++ oracles): exact
mode against the adjoint, finite shots against the fp64 shifted circuits within the shot noise, the stream contract
(determinism, counters, independence of the batch), the shift mask, grouped weights and the module surface."""
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128, QuantumLayer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (pshift_counter, pshift_rows,
                                                                                         qsim, qsim_probs, sample_z,
                                                                                         z_signs)

SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32


def inputs(n, L, B, G=0):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if G == 0 else torch.rand(G, L, n, 2) * 2 * math.pi
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(2)) * 2 - 1
    return x, w, gE


def grads(x, w, gE, **kw):
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    (qsim(xa, wa, "cpu", **kw) * gE).sum().backward()
    return xa.grad, wa.grad


def shifted_reference(x, w, gE):
    """(G_exact, sigma1) (B, P) fp64 from the fp64 probabilities of the 2P shifted circuits: the exact parameter-shift
    gradient and the standard deviation of its one-shot-per-circuit estimate -- sigma^2 = (Var+ + Var-) / 4 with
    Var+- = p . v^2 - (p . v)^2, v = z_signs @ gE[b], the per-shot variance including the wires' correlations."""
    B, n = x.shape
    P = 2 * n * w.shape[-3]
    v = gE.double() @ z_signs(n, dtype=torch.float64).T   # (B, D)
    G = torch.zeros(B, P, dtype=torch.float64)
    var = torch.zeros(B, P, dtype=torch.float64)
    for p in range(P):
        m = []
        for sh in (0.5 * math.pi, -0.5 * math.pi):
            ws = w.clone()
            ws.view(-1, P)[:, p] += sh
            pr = qsim_probs(x, ws, "cpu")
            m.append((pr * v).sum(1))
            var[:, p] += (pr * v * v).sum(1) - m[-1] ** 2
        G[:, p] = 0.5 * (m[0] - m[1])
    return G, (var.clamp_min(0) / 4).sqrt()


@pytest.mark.parametrize("n,L,B", [(2, 1, 3), (5, 3, 3), (8, 3, 4)])
def test_exact_mode_equals_adjoint(n, L, B):
    x, w, gE = inputs(n, L, B)
    dx_a, dw_a = grads(x, w, gE)
    dx, dw = grads(x, w, gE, diff_method="parameter_shift", shots=None)
    ex, ew = float((dx - dx_a).abs().max()), float((dw - dw_a).abs().max())
    print(f"n={n} L={L} B={B}: |dx - adjoint|={ex:.2e} |dw - adjoint|={ew:.2e}")
    assert dx.shape == x.shape and dw.shape == w.shape
    assert ex <= 1e-6 and ew <= 1e-6


@pytest.mark.parametrize("n,L,B,shots", [(2, 1, 3, 257), (8, 3, 4, 256), (12, 2, 2, 1024)])
def test_finite_shots_within_shot_noise(n, L, B, shots):
    x, w, gE = inputs(n, L, B)
    G_exact, sigma1 = shifted_reference(x, w, gE)
    G = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI).double()
    bound = 6 * sigma1 / math.sqrt(shots) + 4 * gE.double().abs().sum(1, keepdim=True) / shots
    ratio = float(((G - G_exact).abs() / bound).max())
    print(f"n={n} L={L} B={B} shots={shots}: max |G - G_exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert float((G - G_exact).abs().max()) > 0   # (shots were drawn)
    # the autograd path is the same rows: dx the layer-0 RY columns, dw their sum over the samples
    dx, dw = grads(x, w, gE, diff_method="parameter_shift", shots=shots, seed=SEED_HI, counter=CTR_HI)
    assert torch.equal(dx, G[:, 0:2 * n:2].float())
    assert torch.allclose(dw.reshape(-1).double(), G.sum(0), rtol=0, atol=1e-5)


def test_rows_are_the_samplers_streams():
    """Circuit (p, s) is sample_z of its probabilities under counter c + ((1 + 2p + s) << 48) (mod 2^64)."""
    n, L, B, shots = 5, 2, 3, 65
    x, w, gE = inputs(n, L, B)
    G = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    P = 2 * n * L
    assert pshift_counter(CTR_HI, 0, 0) == CTR_HI + (1 << 48)
    assert pshift_counter((1 << 64) - 1, P - 1, 1) == ((1 << 64) - 1 + ((2 * P) << 48)) % (1 << 64)
    for p in (0, 7, P - 1):
        E = []
        for s, sh in enumerate((0.5 * math.pi, -0.5 * math.pi)):
            ws = w.clone()
            ws.view(-1)[p] += sh
            E.append(sample_z(qsim_probs(x, ws, "cpu"), shots, SEED_HI, pshift_counter(CTR_HI, p, s)).double())
        assert torch.equal(G[:, p], (gE.double() * (E[0] - E[1]) * 0.5).sum(1).float())


def test_determinism_counters_and_batch_independence():
    n, L, shots = 5, 3, 256
    x, w, gE = inputs(n, L, 4)
    kw = dict(diff_method="parameter_shift", shots=shots, seed=SEED_HI)
    a = grads(x, w, gE, counter=CTR_HI, **kw)
    b = grads(x, w, gE, counter=CTR_HI, **kw)
    c = grads(x, w, gE, counter=CTR_HI + 1, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    G4 = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    G1 = pshift_rows(x[:1], w, gE[:1], "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    assert torch.equal(G4[:1], G1)
    # the backward's streams are not the forward's: the forward's value is that of the adjoint call
    E = qsim(x, w, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    assert torch.equal(qsim(x, w, "cpu", counter=CTR_HI, **kw), E)


@pytest.mark.parametrize("shots", [None, 256])
def test_shift_mask(shots):
    n, L, B = 5, 3, 3
    x, w, gE = inputs(n, L, B)
    kw = dict(diff_method="parameter_shift", shots=shots, seed=SEED_HI, counter=CTR_HI)
    dx, dw = grads(x, w, gE, **kw)
    mask = torch.rand(L, n, 2, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[0] = False   # all of layer 0: dx still comes out of its RY circuits
    mask[1, 0, 0] = True
    dxm, dwm = grads(x, w, gE, shift_mask=mask, **kw)
    assert bool(mask.any()) and not bool(mask.all())
    assert torch.equal(dwm[~mask], torch.zeros_like(dwm[~mask]))
    assert torch.equal(dwm[mask], dw[mask]) and float(dw[mask].abs().max()) > 0
    assert torch.equal(dxm, dx)
    # without a gradient for x the masked layer-0 circuits do not run either: same weights' gradient
    wa = w.clone().requires_grad_()
    (qsim(x, wa, "cpu", shift_mask=mask, **kw) * gE).sum().backward()
    assert torch.equal(wa.grad, dwm)


@pytest.mark.parametrize("shots", [None, 256])
def test_grouped_weights(shots):
    n, L, B, Gr = 5, 2, 6, 3
    x, w, gE = inputs(n, L, B, Gr)
    kw = dict(diff_method="parameter_shift", shots=shots, seed=SEED_HI, counter=CTR_HI)
    master = w[0].clone().requires_grad_()
    noise = (w - w[0]).detach()
    w = (master.unsqueeze(0) + noise).detach()   # (the grouped weights the call sees, to the bit)
    xa = x.clone().requires_grad_()
    (qsim(xa, master.unsqueeze(0) + noise, "cpu", **kw) * gE).sum().backward()
    # per group, rows keeping their index in the whole batch
    rows = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    assert torch.equal(xa.grad, rows[:, 0:2 * n:2])
    assert torch.allclose(master.grad.reshape(-1), rows.sum(0), rtol=0, atol=1e-5)
    if shots is None:
        xb, mb = x.clone().requires_grad_(), w[0].clone().requires_grad_()
        (qsim(xb, mb.unsqueeze(0) + noise, "cpu") * gE).sum().backward()
        assert float((xa.grad - xb.grad).abs().max()) <= 1e-6 and float((master.grad - mb.grad).abs().max()) <= 1e-6
    else:   # row b of group g: the ungrouped call on that group's weights, at the same row index
        g = 1
        solo = pshift_rows(x[:4], w[g], gE[:4], "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
        assert torch.equal(rows[2:4], solo[2:4])


def test_modules():
    torch.manual_seed(0)
    keys = list(QSC_P128(4, 2, 3, True, False, 128).state_dict().keys())
    m = QSC_P128(4, 2, 3, True, False, 128, backend="cpu", shots=64, diff_method="parameter_shift")
    assert list(m.state_dict().keys()) == keys
    assert m.qlayer.diff_method == "parameter_shift" and m.qlayer.shift_mask is None
    assert "diff_method=parameter_shift" in repr(m.qlayer)
    assert QuantumLayer(4, 2).diff_method == "adjoint" and "diff_method=adjoint" in repr(QuantumLayer(4, 2))

    layer = QuantumLayer(4, 2, "cpu", shots=64, diff_method="parameter_shift")
    layer.manual_shot_seed(5)
    x, _, gE = inputs(4, 2, 3)
    xa = x.clone().requires_grad_()
    (layer(xa) * gE).sum().backward()
    dx, dw = grads(x, layer.weights.detach(), gE, diff_method="parameter_shift", shots=64, seed=5, counter=0)
    assert torch.equal(xa.grad, dx) and torch.equal(layer.weights.grad, dw)
    # the mask and the method are attributes
    layer.weights.grad = None
    layer.shift_mask = torch.zeros(2, 4, 2, dtype=torch.bool)
    layer.shift_mask[1, 2, 0] = True
    (layer(x) * gE).sum().backward()
    assert int((layer.weights.grad != 0).sum()) == 1 and float(layer.weights.grad[1, 2, 0]) != 0
    layer.diff_method, layer.shift_mask, layer.shots = "adjoint", None, None
    layer.weights.grad = None
    (layer(x) * gE).sum().backward()
    assert torch.equal(layer.weights.grad, grads(x, layer.weights.detach(), gE)[1])

    m.train()
    inp = torch.randn(2, 2, 16, 8)
    m(inp).sum().backward()
    assert m.qlayer.weights.grad is not None and bool(torch.isfinite(m.qlayer.weights.grad).all())
    assert m.preprocess[0].weight.grad is not None


def test_classifier_step_with_per_stream_noise():
    """The ungraphed ClassifierStep.forward: one noise draw per stream through grouped weights."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep
    torch.manual_seed(0)
    m = QSC_P128(4, 2, 3, True, False, 128, backend="cpu", shots=64, diff_method="parameter_shift").train()
    m.qlayer.shift_mask = torch.ones(2, 4, 2, dtype=torch.bool)
    m.qlayer.shift_mask[1, :, 1] = False
    step = ClassifierStep(m, n_streams=3)
    logp = step.forward(torch.randn(6, 2, 16, 8))
    torch.nn.functional.nll_loss(logp, torch.arange(6) % 3).backward()
    g = m.qlayer.weights.grad
    assert g.shape == (2, 4, 2) and bool(torch.isfinite(g).all())
    assert float(g[1, :, 1].abs().max()) == 0 and float(g[:, :, 0].abs().min()) > 0
    assert m.preprocess[0].weight.grad is not None


def test_value_errors():
    x, w, _ = inputs(4, 2, 2)
    with pytest.raises(ValueError, match="diff_method"):
        qsim(x, w, "cpu", diff_method="backprop")
    with pytest.raises(ValueError, match="torch"):
        qsim(x, w, "torch", diff_method="parameter_shift")
    with pytest.raises(ValueError, match="shift_mask"):
        qsim(x, w, "cpu", diff_method="parameter_shift", shift_mask=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="shift_mask"):
        qsim(x, w, "cpu", shift_mask=torch.ones(2, 4, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="2\\^16"):
        qsim(torch.zeros(1, 2), torch.zeros(8192, 2, 2), "cpu", diff_method="parameter_shift")
    with pytest.raises(ValueError, match="shots"):
        qsim(x, w, "cpu", diff_method="parameter_shift", shots=(1 << 20) + 1)
