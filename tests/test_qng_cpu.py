"""Quantum natural gradient (ops/qng.py): the float64 metric oracle against the diagonal blocks of the full
Fubini-Study metric from an autograd Jacobian, the blocks' structure, the CPU preconditioner against
torch.linalg.solve, the refusals and the runner plumbing.  CPU only."""
import functools
import math
import warnings

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qng import QNGPreconditioner, metric_tensor
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import ring_inverse_index

F64, C128 = torch.float64, torch.complex128
SHAPES = [(2, 1), (3, 2), (4, 3), (5, 2)]
B = 3


def inputs(n, L, batch=B):
    g = torch.Generator().manual_seed(100 * n + L)
    x = torch.rand(batch, n, generator=g, dtype=F64) * 2 - 1
    w = torch.rand(L, n, 2, generator=g, dtype=F64) * 2 * math.pi
    return x, w


def one_qubit(state, q, u):
    """The 2 x 2 complex matrix u on wire q (bit q of the basis index) of a (2^n,) state."""
    D = state.shape[0]
    v = state.view(D >> (q + 1), 2, 1 << q)
    return torch.einsum("ab,ibj->iaj", u, v).reshape(D)


def state_of(xs, w, perm):
    """The circuit's final state (2^n,) complex128 of one sample, a function of the (L, n, 2) angles: RY(x_q) then
    per layer RY, RZ on every wire and the CNOT ring.  Written out gate by gate, embedding apart from layer 0."""
    L, n, _ = w.shape
    s = torch.zeros(1 << n, dtype=C128)
    s[0] = 1.0

    def ry(t):
        c, sn = torch.cos(t / 2).to(C128), torch.sin(t / 2).to(C128)
        return torch.stack([torch.stack([c, -sn]), torch.stack([sn, c])])

    def rz(t):
        e = torch.complex(torch.cos(t / 2), -torch.sin(t / 2))
        z = torch.zeros((), dtype=C128)
        return torch.stack([torch.stack([e, z]), torch.stack([z, e.conj()])])

    for q in range(n):
        s = one_qubit(s, q, ry(xs[q]))
    for l in range(L):
        for q in range(n):
            s = one_qubit(s, q, ry(w[l, q, 0]))
        for q in range(n):
            s = one_qubit(s, q, rz(w[l, q, 1]))
        s = s[perm]
    return s


@functools.lru_cache(maxsize=None)
def full_metric_blocks(n, L):
    """(B, 2L, n, n): the diagonal blocks of Re<d_i psi|d_j psi> - Re(<d_i psi|psi><psi|d_j psi>) per sample."""
    x, w = inputs(n, L)
    perm = ring_inverse_index(n)
    P = 2 * n * L
    out = torch.empty(B, 2 * L, n, n, dtype=F64)
    for b in range(B):
        f = lambda wf: torch.view_as_real(state_of(x[b], wf.view(L, n, 2), perm)).reshape(-1)   # noqa: E731
        J = torch.autograd.functional.jacobian(f, w.reshape(-1).clone())          # (2 D, P) real
        J = torch.view_as_complex(J.reshape(-1, 2, P).permute(0, 2, 1).contiguous())   # (D, P)
        psi = state_of(x[b], w, perm)
        ov = psi.conj() @ J                                                        # <psi|d_j psi>
        g = (J.conj().T @ J).real - (ov.conj()[:, None] * ov[None, :]).real        # (P, P)
        g = g.view(L, n, 2, L, n, 2)
        for l in range(L):
            for k in range(2):
                out[b, 2 * l + k] = g[l, :, k, l, :, k]
    return out


@pytest.mark.parametrize("n,L", SHAPES)
def test_oracle_is_the_block_diagonal_fubini_study_metric(n, L):
    x, w = inputs(n, L)
    got = metric_tensor(x, w, "cpu", per_sample=True)
    assert got.dtype == F64 and tuple(got.shape) == (B, 2 * L, n, n)
    ref = full_metric_blocks(n, L)
    err = float((got - ref).abs().max())
    print(f"n={n} L={L}: max |metric - Fubini-Study block| = {err:.3g}")
    assert err <= 1e-12
    assert float((metric_tensor(x, w, "cpu") - ref.mean(0)).abs().max()) <= 1e-12


@pytest.mark.parametrize("n,L", SHAPES)
def test_block_structure(n, L):
    x, w = inputs(n, L)
    g = metric_tensor(x, w, "cpu", per_sample=True)
    assert float((g - g.transpose(-1, -2)).abs().max()) <= 1e-15
    assert float(torch.linalg.eigvalsh(g).min()) >= -1e-12
    # the diagonal is (1 - m_i^2) / 4 <= 1 / 4, m the expectation of the wire's Y (RY blocks) or Z (RZ blocks)
    d = torch.diagonal(g, dim1=-2, dim2=-1)
    assert float(d.max()) <= 0.25 + 1e-12 and float(d.min()) >= -1e-12
    # RZ blocks: m is <Z> of the state behind the layer's RY gates; for layer 0 that is the product state
    th = x + w[0, :, 0]
    m0 = torch.cos(th)
    assert float((d[:, 1] - 0.25 * (1 - m0 ** 2)).abs().max()) <= 1e-12
    assert float((g[:, 0] - 0.25 * torch.eye(n, dtype=F64)).abs().max()) <= 1e-15
    assert float((g[:, 1] - torch.diag_embed(0.25 * torch.sin(th) ** 2)).abs().max()) <= 1e-12


@pytest.mark.parametrize("n,L", SHAPES)
def test_diagonal_is_a_quarter_of_one_minus_the_mean_squared(n, L):
    """Every block's diagonal against the means of its own measurement: <Z_i> of the state behind the RY gates (from
    the project's probabilities of a circuit cut there), so an error in the walk's state shows."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import z_signs
    x, w = inputs(n, L)
    g = metric_tensor(x, w, "cpu", per_sample=True)
    perm = ring_inverse_index(n)
    zs = z_signs(n, dtype=F64)
    for l in range(L):
        # the circuit up to layer l's RY gates: layers < l whole, layer l with RZ = 0 and its ring undone
        wc = w[:l + 1].clone()
        wc[l, :, 1] = 0.0
        for b in range(B):
            psi = state_of(x[b], wc, perm)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(perm.numel())
            p = (psi.abs() ** 2)[inv]
            m = p @ zs
            d = torch.diagonal(g[b, 2 * l + 1])
            assert float((d - 0.25 * (1 - m ** 2)).abs().max()) <= 1e-12


def test_cpu_preconditioner_is_the_block_solve():
    n, L, lam = 4, 3, 0.01
    x, w = inputs(n, L, batch=5)
    x32, w32 = x.float(), w.float()
    grad = torch.randn(L, n, 2, generator=torch.Generator().manual_seed(3))
    g = metric_tensor(x32, w32, "cpu")
    ref = torch.empty(L, n, 2, dtype=F64)
    for l in range(L):
        for k in range(2):
            A = g[2 * l + k] + lam * torch.eye(n, dtype=F64)
            ref[l, :, k] = torch.linalg.solve(A, grad[l, :, k].double())
    got = grad.clone()
    out = QNGPreconditioner(n, L, lam).precondition(got, x32, w32)
    assert out is got and got.dtype == torch.float32
    # (1e-10 on the float64 solve; the result is then rounded to fp32 once)
    assert float((got.double() - ref).abs().max()) <= 1e-10 + 2.0 ** -24 * float(ref.abs().max())
    # a huge lam swamps the metric (|g| <= 1 / 4): grad / lam
    big = grad.clone()
    QNGPreconditioner(n, L, 1e6).precondition(big, x32, w32)
    assert float(((big.double() - grad.double() / 1e6).abs() / (grad.double().abs() / 1e6)).max()) <= 1e-5


def test_refusals(tmp_path, monkeypatch):
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam"):
            QNGPreconditioner(3, 2, lam)
    x, w = (t.float() for t in inputs(3, 2))
    q = QNGPreconditioner(3, 2, 0.01)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 2, 2), torch.zeros(2, 3, 2, dtype=F64), torch.zeros(12)):
        with pytest.raises(ValueError, match="grad"):
            q.precondition(bad, x, w)
    with pytest.raises(ValueError):
        q.precondition(torch.zeros(2, 3, 2), x[:, :2], w)
    with pytest.raises(ValueError):
        metric_tensor(x, w.unsqueeze(0).repeat(3, 1, 1, 1), "cpu")   # grouped weights: the metric is the master's
    with pytest.raises(ValueError):
        metric_tensor(x, w, "torch")
    with pytest.raises(RuntimeError):
        metric_tensor(x, w, "hip")   # CPU tensors
    # more than one rank: the batch metric would need a collective -- refused, not half-built
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner
    r = Y2HRunner(n_epochs=1, data_len=60, batch_size_DML=16, device="cpu", workspace=str(tmp_path / "y"),
                  data_dir=str(tmp_path / "data"), n_qubits=3, n_layers=2, qsc_qng=True)
    monkeypatch.setattr(r._context(), "world", 2)   # (restored: the context outlives the runner)
    with pytest.raises(ValueError, match="world size 1"):
        r.qsc_qng_preconditioner(None)
    r.qsc_qng = False
    assert r.qsc_qng_preconditioner(None) is None


def test_runner_trains_with_qng_on_cpu(tmp_path):
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner

    def run(tag, **kw):
        r = Y2HRunner(n_epochs=1, data_len=40, batch_size_DML=16, device="cpu", workspace=str(tmp_path / tag),
                      data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=3, n_layers=2, use_quantumnat=False,
                      seed=0, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = r.train_QSC_P128()
        return r, {k: v.detach().clone() for k, v in m.state_dict().items()}

    r0, plain = run("plain")
    r1, off = run("off", qsc_qng=False)
    r2, on = run("on", qsc_qng=True, qsc_qng_lambda=0.01)
    assert all(math.isfinite(v) for v in r2.train_QSC_losses + r2.val_QSC_losses) and len(r2.train_QSC_losses) == 1
    assert all(bool(torch.isfinite(v).all()) for v in on.values())
    assert not torch.equal(on["qlayer.weights"], plain["qlayer.weights"])
    assert list(off) == list(plain) and all(torch.equal(off[k], plain[k]) for k in plain)
    assert r1.train_QSC_losses == r0.train_QSC_losses and r1.val_QSC_losses == r0.val_QSC_losses
