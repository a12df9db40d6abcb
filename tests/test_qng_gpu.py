"""The metric-tensor and natural-gradient kernels (csrc/hip/qsim_metric.hip, ops/qng.py): every entry of the
per-sample rows against the float64 oracle within the derived fp32 bound, the exact properties (symmetry, layer 0's
I / 4, independence of the batch and of the launcher's split), the Cholesky solve within Higham's bound and in place
inside a larger buffer, graph capture, LDS poisoning, the entry points' refusals and the training step's hook."""
import ctypes
import functools
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import qng as QN
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace, make_optimizer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qng import QNGPreconditioner, metric_tensor
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import reduce_slab
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep

pytestmark = pytest.mark.gpu

# (n, L, B): D below the workgroup size, the 16-padding of the MFMA operand at small n, the register / LDS boundary
# of the simulators, the largest state; B = 1 and B = 300 at n = 8: one workgroup per (sample, layer) and per sample
CASES = [(2, 1, 3), (5, 3, 3), (8, 3, 4), (10, 2, 2), (12, 2, 2), (12, 3, 1), (8, 3, 1), (8, 3, 300)]
SENTINEL = -7.0
INVALID = 1   # hipErrorInvalidValue
_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def entry_bound(n, L):
    """Per entry of g = (C - m m^T) / 4: the L1 error of the fp32 probabilities, 2^-19 per rotation (the project's
    bound, tests/test_shots_stream_gpu.py) over at most 2 n (l + 1) + 2 n <= 2 n (L + 1) rotations, through
    (|dC| + 2 |dm|) / 4; plus docs/PARITY.md's (K + 2) 2^-24 S for an fp32 sum of K = 2^n products in any order,
    S = sum p = 1."""
    return 0.75 * n * (L + 1) * 2.0 ** -17 + 0.25 * ((1 << n) + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(n, L, B):
    """Host inputs (fp32) and the float64 oracle (B, 2L, n, n)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * L + 1)
    x = torch.rand(B, n, generator=g) * 2 - 1
    w = torch.rand(L, n, 2, generator=g) * 2 * math.pi
    return x, w, metric_tensor(x, w, "cpu", per_sample=True)


def rows_of(x, w, fill=None):
    B, n = x.shape
    L = w.shape[0]
    rows = torch.empty(B, 2 * L * n * n, device=x.device) if fill is None else \
        torch.full((B, 2 * L * n * n), fill, device=x.device)
    return QN.hip_metric_rows(x, w, rows)


@pytest.mark.parametrize("n,L,B", CASES)
def test_rows_against_the_oracle(cuda, n, L, B):
    x, w, ref = case(n, L, B)
    rows = rows_of(x.to(cuda), w.to(cuda), fill=SENTINEL).view(B, 2 * L, n, n)
    err = (rows.cpu().double() - ref).abs()
    bound = entry_bound(n, L)
    print(f"qng rows n={n} L={L} B={B}: worst |g - g64| = {float(err.max()):.3e}, bound {bound:.3e}, "
          f"ratio {float(err.max()) / bound:.4f}")
    assert bool((err <= bound).all())
    # exact: symmetric blocks, layer 0's RY block
    assert torch.equal(rows, rows.transpose(-1, -2))
    assert torch.equal(rows[:, 0], (0.25 * torch.eye(n, device=cuda)).expand(B, n, n))
    # the public op: per-sample rows, and their mean
    assert torch.equal(metric_tensor(x.to(cuda), w.to(cuda), per_sample=True), rows)
    mean = metric_tensor(x.to(cuda), w.to(cuda))
    assert tuple(mean.shape) == (2 * L, n, n) and mean.dtype == torch.float32
    # (the fp32 sum of B entries of size <= 1 / 4 + bound, and the division)
    assert float((mean.cpu().double() - ref.mean(0)).abs().max()) <= bound + (B + 1) * 2.0 ** -24 * (0.25 + bound)


@pytest.mark.parametrize("n,L,B", [(8, 3, 300), (8, 3, 4), (12, 2, 2), (5, 3, 3)])
def test_a_row_does_not_depend_on_the_batch(cuda, n, L, B):
    """B = 300 walks each sample's circuit in one workgroup, B = 1 splits it over the layers: the same bits."""
    x, w, _ = case(n, L, B)
    xd, wd = x.to(cuda), w.to(cuda)
    rows = rows_of(xd, wd)
    for b in sorted({0, B // 2, B - 1}):
        assert torch.equal(rows_of(xd[b:b + 1].contiguous(), wd)[0], rows[b])


@pytest.mark.parametrize("lam", [1e-2, 1.0])
@pytest.mark.parametrize("n,L,B", [(2, 1, 3), (5, 3, 3), (8, 3, 4), (12, 2, 2)])
def test_solve(cuda, n, L, B, lam):
    """Against the float64 solve of the kernel's own fp32 gsum: Higham's backward error of a Cholesky solve,
    n gamma_{3n+1}, times cond_2(A), a factor 2 for the right-hand side and second order.  In place on a view into a
    larger sentinel-filled buffer: nothing outside the 2 n L floats changes."""
    x, w, _ = case(n, L, B)
    rows = rows_of(x.to(cuda), w.to(cuda))
    gsum = reduce_slab(rows, torch.empty(rows.shape[1], device=cuda))
    P = 2 * n * L
    flat = torch.full((P + 64,), SENTINEL, device=cuda)
    grad = flat[24:24 + P].view(L, n, 2)
    g0 = torch.randn(L, n, 2, generator=torch.Generator().manual_seed(5))
    grad.copy_(g0)
    QN.hip_qng_solve(gsum, B, lam, grad)
    torch.cuda.synchronize()
    assert bool((flat[:24] == SENTINEL).all()) and bool((flat[24 + P:] == SENTINEL).all())
    A = gsum.cpu().double().view(2 * L, n, n) / B + lam * torch.eye(n, dtype=torch.float64)
    worst = 0.0
    for l in range(L):
        for k in range(2):
            Ab = A[2 * l + k]
            ref = torch.linalg.solve(Ab, g0[l, :, k].double())
            ev = torch.linalg.eigvalsh(Ab)
            cond = float(ev[-1] / ev[0])
            rel = float((grad[l, :, k].cpu().double() - ref).norm() / ref.norm())
            bound = 2 * n * (3 * n + 1) * 2.0 ** -24 * cond
            worst = max(worst, rel / bound)
            assert rel <= bound, (l, k, rel, bound)
    print(f"qng solve n={n} L={L} B={B} lam={lam}: worst (relative error / bound) = {worst:.4f}")


def test_preconditioner_is_its_three_launches(cuda):
    n, L, B = 8, 3, 4
    x, w, _ = case(n, L, B)
    xd, wd = x.to(cuda), w.to(cuda)
    g0 = torch.randn(L, n, 2, generator=torch.Generator().manual_seed(6)).to(cuda)
    q = QNGPreconditioner(n, L, 0.01, cuda)
    got = q.precondition(g0.clone(), xd, wd)
    gsum = reduce_slab(rows_of(xd, wd), torch.empty(2 * L * n * n, device=cuda))
    ref = g0.clone()
    QN.hip_qng_solve(gsum, B, 0.01, ref)
    assert torch.equal(got, ref) and not torch.equal(got, g0)
    # a NaN sample poisons its blocks' pivots: those blocks' gradients stay as they were
    xn = xd.clone()
    xn[1, 2] = float("nan")
    kept = q.precondition(g0.clone(), xn, wd)
    assert torch.equal(kept[:, :, 1], g0[:, :, 1]) and torch.equal(kept[1:, :, 0], g0[1:, :, 0])
    assert torch.equal(kept[0, :, 0], ref[0, :, 0])   # layer 0's RY block is I / 4 whatever the angles
    with pytest.raises(NotImplementedError, match="12"):
        QNGPreconditioner(13, 1, 0.01, cuda)
    with pytest.raises(NotImplementedError, match="12"):
        metric_tensor(torch.zeros(1, 13, device=cuda), torch.zeros(1, 13, 2, device=cuda))


def test_graph_capture(cuda):
    n, L, B = 8, 3, 4
    q = QNGPreconditioner(n, L, 0.01, cuda)
    q.reserve(B)
    x, w, grad = torch.zeros(B, n, device=cuda), torch.zeros(L, n, 2, device=cuda), torch.zeros(L, n, 2, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q.precondition(grad, x, w)   # (warm-up: every launcher declared, every workspace there)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q.precondition(grad, x, w)
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        xs, ws, gs = torch.rand(B, n, generator=g) * 2 - 1, torch.rand(L, n, 2, generator=g) * 6, torch.randn(L, n, 2, generator=g)
        x.copy_(xs)
        w.copy_(ws)
        grad.copy_(gs)
        graph.replay()
        torch.cuda.synchronize()
        eager = QNGPreconditioner(n, L, 0.01, cuda).precondition(gs.to(cuda), xs.to(cuda), ws.to(cuda))
        assert torch.equal(grad, eager) and not torch.equal(grad, gs.to(cuda))


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF, 0x7F7FFFFF])   # (as test_pshift_gpu.py, and a huge finite value)
@pytest.mark.parametrize("n,L,B", [(5, 3, 3), (8, 3, 4), (12, 2, 2)])
def test_lds_poison(cuda, n, L, B, pattern):
    x, w, _ = case(n, L, B)
    xd, wd = x.to(cuda), w.to(cuda)
    g0 = torch.randn(L, n, 2, generator=torch.Generator().manual_seed(7)).to(cuda)

    def run():
        rows = rows_of(xd, wd)
        return rows, QNGPreconditioner(n, L, 0.01, cuda).precondition(g0.clone(), xd, wd)

    clean = run()
    try:
        nat.set_lds_poison(pattern)
        poisoned = run()
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    for a, b in zip(clean, poisoned):
        assert torch.equal(a, b)


def test_entry_point_refusals(cuda):
    lib = nat.hip_lib()
    metric = nat.fn(lib, "qd_qsim_metric", [_p, _p, _p, _i, _i, _i, _p])
    solve = nat.fn(lib, "qd_qng_solve", [_p, _i, _f, _p, _i, _i, _p])
    st = nat.stream_ptr(cuda)
    x, w = torch.zeros(4, 13, device=cuda), torch.zeros(4, 13, 2, device=cuda)
    rows = torch.full((4 * 2 * 4 * 13 * 13,), SENTINEL, device=cuda)
    gsum = torch.full((2 * 4 * 13 * 13,), 0.25, device=cuda)
    grad = torch.full((4 * 13 * 2,), SENTINEL, device=cuda)
    for n, B, L in [(1, 4, 4), (13, 4, 4), (8, 0, 4), (8, 4, 0), (8, -1, 4)]:
        assert metric(nat.ptr(x), nat.ptr(w), nat.ptr(rows), B, n, L, st) == INVALID
        assert solve(nat.ptr(gsum), B, 0.01, nat.ptr(grad), n, L, st) == INVALID
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert solve(nat.ptr(gsum), 4, lam, nat.ptr(grad), 8, 4, st) == INVALID
    assert metric(None, nat.ptr(w), nat.ptr(rows), 4, 8, 4, st) == INVALID
    assert metric(nat.ptr(x), nat.ptr(w), None, 4, 8, 4, st) == INVALID
    assert solve(None, 4, 0.01, nat.ptr(grad), 8, 4, st) == INVALID
    assert solve(nat.ptr(gsum), 4, 0.01, None, 8, 4, st) == INVALID
    torch.cuda.synchronize()
    assert bool((rows == SENTINEL).all()) and bool((grad == SENTINEL).all())


@pytest.mark.parametrize("path", ["module", "fused"])
def test_training_step_hook(cuda, path, monkeypatch):
    """One step of an 8-qubit, 3-layer QSC_P128 through ClassifierStep with the hook, against the same step without
    it followed by QNGPreconditioner.precondition on its gradient: the same bits in the quantum gradient and in
    every parameter behind AdamW."""
    n, L, S, b, lam = 8, 3, 3, 4, 0.01

    def world(hook):
        torch.manual_seed(0)
        m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=True, use_gradient_pruning=False).to(cuda).train()
        space = FlatParamSpace(list(m.named_parameters()), cuda)
        step = ClassifierStep(m, S) if path == "module" else ClassifierStep(m, S, space=space, batch_total=S * b)
        assert (step.hip is None) == (path == "module")
        if hook:
            step.set_qng(QNGPreconditioner(n, L, lam, cuda))
        elif path == "module":
            m.qlayer.keep_input = True   # (the oracle's angles; the fused step keeps its own)
        opt = make_optimizer(space, "adamw", 1e-2, weight_decay=0.01, prune_thr=0.0)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(S * b, 2, 16, 8, generator=g).to(cuda)
        y = torch.randint(0, 3, (S * b,), generator=g).to(cuda)
        torch.manual_seed(1)   # (the module path's QuantumNAT draw)
        space.zero_grad()
        step(x, y)
        return m, space, step, opt

    # the module path's first convolution takes its weight gradient from the vendor library, whose default kernel
    # adds with atomics (two identical steps differed by 5e-10 there): ask for its deterministic one, as a
    # bit-for-bit comparison of two runs must
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m1, sp1, st1, opt1 = world(True)
    raw = m1.qlayer.weights.grad.clone()
    angles = st1.angles
    assert tuple(angles.shape) == (S * b, n) and not angles.requires_grad
    st1.precondition()
    opt1.step()
    m2, sp2, st2, opt2 = world(False)
    assert st2.qng is None
    assert torch.equal(m2.qlayer.weights.grad, raw)
    angles2 = m2.qlayer.last_input if path == "module" else st2.hip.angles
    assert torch.equal(angles2, angles)
    QNGPreconditioner(n, L, lam, cuda).precondition(m2.qlayer.weights.grad, angles2.float().contiguous(),
                                                    m2.qlayer.weights)
    assert not torch.equal(m2.qlayer.weights.grad, raw)
    qgrad = m2.qlayer.weights.grad.clone()
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(m1.qlayer.weights.grad, qgrad)
    assert torch.equal(sp1.grad, sp2.grad) and torch.equal(sp1.flat, sp2.flat)


@pytest.mark.parametrize("step", ["exact", "module", "fused"])
def test_runner_trains_with_qng(cuda, tmp_path, monkeypatch, step):
    """train-qsc with qsc_qng on the GPU: the exact step (fused and graph-captured), and a measured mode on the module
    path and in the fused, graphed step.  The hook runs in every step, inside the capture where there is one."""
    import warnings

    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner
    calls, capturing = [], []
    pre = QNGPreconditioner.precondition

    def spy(self, grad, x, w):
        calls.append(tuple(x.shape))
        capturing.append(torch.cuda.is_current_stream_capturing())
        return pre(self, grad, x, w)

    monkeypatch.setattr(QNGPreconditioner, "precondition", spy)
    knobs = {} if step == "exact" else dict(qsc_diff_method="parameter_shift", qsc_shots=64, qsc_step=step)
    r = Y2HRunner(n_epochs=1, data_len=60, batch_size_DML=16, device="cuda", workspace=str(tmp_path / "w"),
                  data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2, use_quantumnat=True,
                  seed=0, qsc_qng=True, qsc_qng_lambda=0.01, **knobs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = r.train_QSC_P128()
    torch.cuda.synchronize()
    assert len(r.train_QSC_losses) == 1 and math.isfinite(r.train_QSC_losses[0]) and math.isfinite(r.val_QSC_losses[0])
    assert bool(torch.isfinite(m.qlayer.weights).all())
    assert calls and all(s[1] == 4 for s in calls)
    assert any(capturing) == (step != "module")   # graphed steps capture the hook; the module path runs it eagerly
