"""On-chip gradients on the host: the ``cpu`` backend against the composition of the oracles written out here, the
parameter-shift rule under noise against a dense fp64 density-matrix derivative (with a derived, not tuned, bound),
the ``diff_method="on_chip"`` API, and the runner's qsc_* training knobs."""
import math
import warnings

import numpy as np
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128, QuantumLayer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (DIFF_METHODS, NoiseModel,
                                                                                         noise_sites, pauli_frames,
                                                                                         pshift_counter, pshift_rows,
                                                                                         qsim, qsim_probs,
                                                                                         sample_z_noisy)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner

SEED_HI = 0x9E3779B97F4A7C15
CTR_HI = (1 << 32) + (1 << 40) + 77
NOISE = NoiseModel(p1=0.05, p2=0.1, readout01=0.02, readout10=0.03)


def inputs(n, L, B):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(2)) * 2 - 1
    return x, w, gE


# ------------------------------------------------------------------------------- 1. the cpu backend
def test_cpu_backend_is_the_host_composition():
    n, L, B, T, shots = 4, 2, 3, 4, 64
    x, w, gE = inputs(n, L, B)
    P = 2 * n * L
    G = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI, noise=NOISE, trajectories=T)
    want = torch.zeros(B, P, dtype=torch.float64)
    xr = x.repeat_interleave(T, dim=0)
    for p in range(P):
        E = []
        for s, sh in enumerate((0.5 * math.pi, -0.5 * math.pi)):
            c = pshift_counter(CTR_HI, p, s)
            F = pauli_frames(noise_sites(NOISE, B, n, L, T, SEED_HI, c))
            ws = w.clone()
            ws.view(-1)[p] += sh
            pr = qsim_probs(xr, ws, "cpu", frames=F.view(B * T, L, 2)).view(B, T, 1 << n)
            E.append(sample_z_noisy(pr, F[:, :, L - 1, 0], NOISE, shots, SEED_HI, c).double())
        want[:, p] = (gE.double() * (E[0] - E[1]) * 0.5).sum(1)
    assert torch.equal(G, want.float())
    assert float(G.abs().max()) > 0
    # all rates zero: the noiseless parameter-shift rows, whatever T
    plain = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI)
    zero = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI, noise=NoiseModel(), trajectories=T)
    assert torch.equal(zero, plain) and not torch.equal(G, plain)


# ------------------------------------------------------------------------------- 2. the rule against the channel
I2 = np.eye(2, dtype=complex)
PAULI = [I2, np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]]),
         np.array([[1, 0], [0, -1]], dtype=complex)]   # I, X, Y, Z


def full_op(U, q, n):
    """The 2^n matrix of the one-qubit U on wire q (wire i = bit i of the basis index)."""
    ops = [U if i == q else I2 for i in range(n)]
    out = ops[n - 1]
    for i in range(n - 2, -1, -1):   # (np.kron's left factor is the more significant one)
        out = np.kron(out, ops[i])
    return out


def cnot_op(c, t, n):
    D = 1 << n
    M = np.zeros((D, D), dtype=complex)
    for k in range(D):
        M[k ^ (((k >> c) & 1) << t), k] = 1
    return M


def ry(a):
    return np.array([[math.cos(a / 2), -math.sin(a / 2)], [math.sin(a / 2), math.cos(a / 2)]], dtype=complex)


def rz(a):
    return np.array([[np.exp(-0.5j * a), 0], [0, np.exp(0.5j * a)]])


def density_matrix_gradient(x, w, gE, n, L, p1, p2, r01, r10):
    """d/dw[l, q, k] of sum_j gE_j <Z_j> of the noisy device, (L, n, 2): the density matrix through every gate, the
    Pauli channel after each fused one-qubit gate and each CNOT, then the per-wire readout confusion.  The derivative
    enters at the parameter's rotation as -i/2 [sigma, rho] (sigma = Y for the RY angle, Z for the RZ angle) and is
    carried through the remaining, linear, maps."""
    D = 1 << n
    bits = (np.arange(D)[:, None] >> np.arange(n)[None, :]) & 1
    read = np.where(bits == 1, -(1 - 2 * r10), 1 - 2 * r01)   # the mean reading of a wire in state 0 / 1
    one = [[full_op(PAULI[c], q, n) for c in range(1, 4)] for q in range(n)]
    two = [[full_op(PAULI[c >> 2], q, n) @ full_op(PAULI[c & 3], (q + 1) % n, n) for c in range(1, 16)]
           for q in range(n)]

    def conj(M, r):
        return M @ r @ M.conj().T

    def channel(r, ops, p):
        return (1 - p) * r + (p / len(ops)) * sum(conj(P, r) for P in ops)

    grad = np.zeros((L, n, 2))
    for lp in range(L):
        for qp in range(n):
            for kp in range(2):
                rho = np.zeros((D, D), dtype=complex)
                rho[0, 0] = 1
                d = None
                for l in range(L):
                    for q in range(n):
                        Ay = full_op(ry(w[l, q, 0]) @ (ry(x[q]) if l == 0 else I2), q, n)
                        Az = full_op(rz(w[l, q, 1]), q, n)
                        if d is not None:
                            d = conj(Az @ Ay, d)
                        if (l, q) == (lp, qp):
                            sig = full_op(PAULI[2 if kp == 0 else 3], q, n)
                            mid = conj(Ay, rho) if kp == 0 else conj(Az @ Ay, rho)
                            d = -0.5j * (sig @ mid - mid @ sig)
                            if kp == 0:
                                d = conj(Az, d)
                        rho = conj(Az @ Ay, rho)
                        rho = channel(rho, one[q], p1)
                        if d is not None:
                            d = channel(d, one[q], p1)
                    for q in range(n):
                        M = cnot_op(q, (q + 1) % n, n)
                        rho = channel(conj(M, rho), two[q], p2)
                        if d is not None:
                            d = channel(conj(M, d), two[q], p2)
                assert abs(np.real(np.trace(rho)) - 1) < 1e-12 and abs(np.trace(d)) < 1e-12
                grad[lp, qp, kp] = float(np.real(np.diag(d)) @ read @ gE)
    return grad


def test_density_matrix_gradient_is_the_adjoint_without_noise():
    """The reference itself, against autograd of the exact simulator."""
    n, L = 3, 2
    x, w, gE = inputs(n, L, 1)
    wa = w.clone().requires_grad_()
    (qsim(x, wa, "torch") * gE).sum().backward()   # (fp32)
    got = density_matrix_gradient(x[0].double().numpy(), w.double().numpy(), gE[0].double().numpy(), n, L, 0, 0, 0, 0)
    assert np.abs(got - wa.grad.double().numpy()).max() <= 2e-5 * float(gE.abs().sum())   # the project's fp32 tolerance


def test_parameter_shift_under_noise_against_the_density_matrix():
    """Bound: Var(E_j^+-) <= 1/T + 1/shots (total variance over trajectories and shots), so std(G) <= sum|gE|
    sqrt((1/T + 1/shots) / 2) per row; the B rows are independent; six sigma of their mean."""
    n, L, B, T, shots = 3, 2, 64, 1024, 16384
    p1, p2, r01, r10 = 0.05, 0.1, 0.02, 0.03
    x1, w, g1 = inputs(n, L, 1)
    x, gE = x1.expand(B, n).contiguous(), g1.expand(B, n).contiguous()
    G = pshift_rows(x, w, gE, "cpu", shots=shots, seed=SEED_HI, counter=CTR_HI,
                    noise=NoiseModel(p1, p2, r01, r10), trajectories=T).double()
    args = (x1[0].double().numpy(), w.double().numpy(), g1[0].double().numpy(), n, L)
    want = density_matrix_gradient(*args, p1, p2, r01, r10).reshape(-1)
    ideal = density_matrix_gradient(*args, 0, 0, 0, 0).reshape(-1)
    sg = float(g1.double().abs().sum())
    bound = 6 * sg * math.sqrt((1 / T + 1 / shots) / (2 * B))
    got = G.mean(0).numpy()
    err = np.abs(got - want).max()
    away = np.abs(ideal - want).max()
    print(f"noisy gradient {got}\ndensity matrix {want}\nnoiseless {ideal}\nbound {bound:.5f} = {bound / sg:.5f} sum|gE|; "
          f"max |got - dm| = {err:.5f} ({err / bound:.2f} bounds), max |noiseless - dm| = {away:.5f} "
          f"({away / bound:.1f} bounds); per-row std / sum|gE| = {G.std(0).min() / sg:.4f} .. {G.std(0).max() / sg:.4f} "
          f"(per-row bound {math.sqrt((1 / T + 1 / shots) / 2):.4f})")
    assert err <= bound
    assert away > 3 * bound   # the check has power: the noiseless gradient fails it


# ------------------------------------------------------------------------------- 3. the API
def test_on_chip_api():
    n, L, B = 4, 2, 3
    x, w, gE = inputs(n, L, B)
    assert "on_chip" in DIFF_METHODS
    with pytest.raises(ValueError, match="shots"):
        qsim(x, w, "cpu", diff_method="on_chip")
    with pytest.raises(ValueError, match="shots"):
        qsim(x, w, "cpu", diff_method="on_chip", noise=NOISE)
    with pytest.raises(ValueError, match="torch"):
        qsim(x, w, "torch", shots=64, diff_method="on_chip")
    with pytest.raises(ValueError, match="on_chip"):   # the refusal stays, and now names the way out
        qsim(x, w, "cpu", shots=64, noise=NOISE, diff_method="parameter_shift")
    with pytest.raises(ValueError, match="trajectories"):
        qsim(x, w, "cpu", shots=64, diff_method="on_chip", trajectories=4)
    with pytest.raises(ValueError, match="multiple"):
        qsim(x, w, "cpu", shots=64, diff_method="on_chip", noise=NOISE, trajectories=3)

    def grads(**kw):
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        E = qsim(xa, wa, "cpu", shots=64, seed=SEED_HI, counter=CTR_HI, **kw)
        (E * gE).sum().backward()
        return E.detach(), xa.grad, wa.grad

    # noise=None: "parameter_shift" bit for bit
    for a, b in zip(grads(diff_method="on_chip"), grads(diff_method="parameter_shift")):
        assert torch.equal(a, b)
    # under noise: the noisy forward, and the rows of pshift_rows
    kw = dict(noise=NOISE, trajectories=4)
    E, dx, dw = grads(diff_method="on_chip", **kw)
    assert torch.equal(E, qsim(x, w, "cpu", shots=64, seed=SEED_HI, counter=CTR_HI, **kw))
    G = pshift_rows(x, w, gE, "cpu", shots=64, seed=SEED_HI, counter=CTR_HI, **kw)
    assert torch.equal(dx, G[:, 0:2 * n:2]) and torch.equal(dw.reshape(-1), G.sum(0))
    # shift_mask zeroes dw's entries and leaves dx
    mask = torch.rand(L, n, 2, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[0, 0, 0] = False
    _, dxm, dwm = grads(diff_method="on_chip", shift_mask=mask, **kw)
    assert torch.equal(dxm, dx)
    assert torch.equal(dwm[mask], dw[mask]) and float(dwm[~mask].abs().max()) == 0 and float(dw[~mask].abs().max()) > 0


def test_modules_pass_on_chip_through():
    n, L, B = 4, 2, 3
    x, _, gE = inputs(n, L, B)
    q = QuantumLayer(n, L, "cpu")
    q.shots, q.diff_method, q.noise, q.trajectories = 64, "on_chip", NOISE, 4   # plain attributes
    q.shift_mask = torch.ones(L, n, 2, dtype=torch.bool)
    q.manual_shot_seed(SEED_HI)
    (q(x) * gE).sum().backward()
    G = pshift_rows(x, q.weights.detach(), gE, "cpu", shots=64, seed=SEED_HI, counter=0, noise=NOISE, trajectories=4)
    assert torch.equal(q.weights.grad.reshape(-1), G.sum(0))
    torch.manual_seed(0)
    m = QSC_P128(n_qubits=n, n_layers=L, backend="cpu", shots=64, diff_method="on_chip", noise=NOISE, trajectories=4)
    assert m.qlayer.diff_method == "on_chip" and m.qlayer.noise is NOISE and m.qlayer.trajectories == 4
    torch.nn.functional.nll_loss(m.train()(torch.randn(B, 2, 16, 8)), torch.arange(B) % 3).backward()
    assert float(m.qlayer.weights.grad.abs().max()) > 0 and m.preprocess[0].weight.grad is not None


# ------------------------------------------------------------------------------- 4. the runner's knobs
def _train_qsc(tmp_path, name, **knobs):
    r = Y2HRunner(n_epochs=2, data_len=60, batch_size_DML=16, device="cpu", workspace=str(tmp_path / name),
                  data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2, use_quantumnat=True,
                  seed=0, **knobs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (synthetic-data notice)
        m = r.train_QSC_P128()
    return r, m


def test_runner_trains_on_chip(tmp_path):
    knobs = dict(qsc_diff_method="on_chip", qsc_shots=64, qsc_noise_p1=1e-3, qsc_noise_p2=1e-2, qsc_readout01=0.02,
                 qsc_readout10=0.02, qsc_trajectories=4)
    torch.manual_seed(0)
    w0 = QSC_P128(4, 2, 3).qlayer.weights.detach().clone()   # the runner seeds the same way before building
    r1, m1 = _train_qsc(tmp_path, "a", **knobs)
    r2, m2 = _train_qsc(tmp_path, "b", **knobs)
    assert m1.qlayer.diff_method == "on_chip" and m1.qlayer.shots == 64 and m1.qlayer.trajectories == 4
    assert isinstance(m1.qlayer.noise, NoiseModel) and m1.qlayer.noise.p2 == 1e-2
    assert len(r1.train_QSC_losses) == 2 and all(math.isfinite(v) for v in r1.train_QSC_losses)
    assert r1.train_QSC_losses == r2.train_QSC_losses and r1.val_QSC_losses == r2.val_QSC_losses
    for a, b in zip(m1.state_dict().values(), m2.state_dict().values()):
        assert torch.equal(a, b)
    assert not torch.equal(m1.qlayer.weights.detach().cpu(), w0)


def test_runner_defaults_are_the_old_path(tmp_path):
    r0, m0 = _train_qsc(tmp_path, "absent")
    r1, m1 = _train_qsc(tmp_path, "explicit", qsc_diff_method="adjoint", qsc_shots=0, qsc_noise_p1=0.0,
                        qsc_noise_p2=0.0, qsc_readout01=0.0, qsc_readout10=0.0, qsc_trajectories=1)
    assert r0.qsc_device_knobs() is None and r1.qsc_device_knobs() is None
    assert m0.qlayer.diff_method == "adjoint" and not m0.qlayer.shots and m0.qlayer.noise is None
    assert r0.train_QSC_losses == r1.train_QSC_losses and r0.val_QSC_losses == r1.val_QSC_losses
    assert r0.val_QSC_accuracies == r1.val_QSC_accuracies
    for a, b in zip(m0.state_dict().values(), m1.state_dict().values()):
        assert torch.equal(a, b)


def test_runner_refuses_noise_without_shots(tmp_path):
    r = Y2HRunner(device="cpu", workspace=str(tmp_path / "w"), data_dir=str(tmp_path / "data"), qsc_noise_p1="1e-3")
    assert r.qsc_noise_p1 == 1e-3   # coerced like EvalConfig's
    with pytest.raises(ValueError, match="qsc_shots"):
        r.train_QSC_P128()
    r = Y2HRunner(device="cpu", workspace=str(tmp_path / "w"), data_dir=str(tmp_path / "data"),
                  qsc_diff_method="on_chip")
    with pytest.raises(ValueError, match="shots"):
        r.train_QSC_P128()
