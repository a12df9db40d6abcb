"""The density-matrix adjoint kernel (csrc/hip/qsim_mixed.hip qd_qsim_mixed_adjoint; ops/quantum.py
``mixed_adjoint_rows``, ``qsim_mixed(diff_method="adjoint")``; ops/qsc.py ``QSCStepHIP(exact_noise=True)``): every entry
of G against the float64 shift rule (``mixed_rows`` on ``cpu``, which shares nothing with the adjoint) within a derived
bound, the exact relations (E_out, batch / grid / slot independence, grouped weights, graph replay, LDS poisoning,
sentinels, refusals), zero noise against the exact kernel's adjoint, and the fused step.

The bound (``bound``), derived, not tuned; the terms are tests/test_mixed_gpu.py's.  eps = 2^-24, tau = 2^-21.4.  A
column of G is g = <Lam_m, K rho_m>: rho_m the state behind a rotation, recovered by undoing the later sweeps, Lam_m
the observable carried back to it, K = (-i/2) [P, .] with |<Lam, K rho>| <= ||Lam||_op ||rho||_1.
  * One pass over the 2 n L sweeps moves a trace-norm-1 array by at most
        T1 = n L (7 tau + 2^(n/2) (2^-19 + 2^-21))
    in the trace norm (that file's figure: 7 tau for the four trig values of a rotation, 2^-19 / 2^-21 for the
    round-off of a rotation / CNOT sweep in the Frobenius norm, 2^(n/2) from Frobenius to trace norm).
  * rho_m carries two passes: the recomputed forward and the undo, which has the forward's operations (``mix`` with
    the inverse's constants; e^{-i phi} from the same half-angle values, 2 sqrt(2) tau per entry, within a rotation's
    7 tau).  Every site undone later multiplies an error by at most ||D^-1||_1->1 <= (1 + 2 k) / a = (2 - a) / a
    (one qubit: D^-1 = (id - k I (x) tr_q) / a and ||I (x) tr_q rho||_1 <= 2 ||rho||_1; two qubits the same with
    a + 4 k = 1); A = the product of (2 - a) / a over all 2 n L sites bounds that for every sweep:
        ||d rho_m||_1 <= 2 A T1.
  * Lam_m carries one pass.  D is unital and positive, so it contracts the operator norm, as do the unitaries:
    ||Lam_m||_op <= ||Lam_K||_op = sum_j |gE_j c_j| =: N, a rotation's trig moves it by 7 tau N, and a round-off of
    Frobenius size f ||Lam||_F <= f 2^(n/2) N bounds the operator-norm one:  ||d Lam_m||_op <= N T1.
  * the sum: one term per quad, 8 roundings each, added along a chain of at most ``depth`` = quads per thread and tile
    + 6 (wave) + 2 (waves) + tiles additions; sum |terms| <= ||Lam||_F ||rho||_F <= 2^(n/2) N:
        (depth + 8) eps 2^(n/2) N.
  * the reference: fp32 shifted angles (|w +- pi/2| < 8: 2^-22 per E_j, tests/test_mixed_cpu.py) and its fp32 result:
        (2^-22 + 2^-24) sum_j |gE_j|.
  |dG| <= N T1 (1 + 2 A) + (depth + 8) eps 2^(n/2) N + (2^-22 + 2^-24) sum |gE|.
The accuracy cases (mild per-wire rates, and the README's noise point) keep A <= 4 and need every row's max |G| > 10
bound (checked on the host oracle, before the launch); the cases with rates up to 0.5 use the same formula with their
own A, which makes it wide: they serve the exact relations."""
import ctypes
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace, make_optimizer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, mixed_adjoint_rows,
                                                                                         mixed_readout, mixed_rows,
                                                                                         qsim_mixed)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner, _capture_preserving
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import GraphedStep
from test_mixed_gpu import EPS, TAU, case as inputs, exact_bound, per_wire_noise

pytestmark = pytest.mark.gpu

# (n, L, B, weight groups): rho below the workgroup size, odd sizes, the largest two-array LDS state with grouped
# weights (6), the smallest workspace state (7: 4 tiles), the 16-tile state (8)
CASES = [(2, 1, 3, 0), (3, 2, 5, 0), (4, 3, 2, 0), (6, 2, 3, 3), (7, 2, 2, 0), (8, 2, 2, 0)]
README_CASE = (8, 3, 2, 0)
README_NOISE = NoiseModel(1e-3, 1e-2, 0.02, 0.02)   # the noise point of the README's timing tables
SENTINEL = -7.0
INVALID = 1   # hipErrorInvalidValue
_p, _i = ctypes.c_void_p, ctypes.c_int


class OverHalf(NoiseModel):
    """A model whose thresholds pass 2^31 on one wire (``NoiseModel`` itself admits no rate above 0.5): ``kind`` 1 or 2
    names the gate threshold that does."""

    def __init__(self, kind, **kw):
        super().__init__(**kw)
        self.kind = kind

    def thresholds_host(self, n):
        thr = [t.copy() for t in super().thresholds_host(n)]
        thr[self.kind - 1][n - 1] = (1 << 31) + 1
        return tuple(thr)


def mild_noise(n, L):
    """Unequal rates per wire with a 0 among each kind, scaled so that the amplification A stays below 4
    (log A ~ n L (4/3 max p1 + 16/15 max p2) = 1.04), and a non-trivial readout."""
    return NoiseModel(p1=np.linspace(0.0, 0.3 / (n * L), n), p2=np.linspace(0.6 / (n * L), 0.0, n),
                      readout01=np.linspace(0.0, 0.1, n), readout10=np.linspace(0.2, 0.05, n))


def amplification(noise, n, L):
    thr1, thr2, _ = noise.thresholds_host(n)
    a1 = 1.0 - 4.0 * (thr1.astype(np.float64) / 2.0 ** 32) / 3.0
    a2 = 1.0 - 16.0 * (thr2.astype(np.float64) / 2.0 ** 32) / 15.0
    return float(np.prod((2.0 - a1) / a1) * np.prod((2.0 - a2) / a2)) ** L


def grad_out(n, B):
    """gE: one dominant wire per sample (another wire each), the others small -- Lam sums all of them."""
    g = torch.rand(B, n, generator=torch.Generator().manual_seed(5 + n)) * 0.1 - 0.05
    for b in range(B):
        g[b, b % n] = 1.0 - 0.25 * b
    return g


def bound(n, L, noise, gE, eps=EPS, tau=TAU):
    """(B, 1) fp64: the module docstring's bound per entry of a row."""
    c, _ = mixed_readout(noise, n)
    N = (gE.double().abs() * c.abs()).sum(1, keepdim=True)
    T1 = n * L * (7 * tau + 2.0 ** (n / 2) * (32 + 8) * eps)   # (2^-19 + 2^-21 = 40 eps in fp32)
    A = amplification(noise, n, L)
    quads = 4 ** (n - 1)
    tiles = 1 if n <= 6 else 4 ** (n - 6)
    depth = max(1, min(quads, 1024) // 256) + 6 + 2 + tiles
    return N * T1 * (1 + 2 * A) + (depth + 8) * eps * 2.0 ** (n / 2) * N + \
        (2.0 ** -22 + 2.0 ** -24) * gE.double().abs().sum(1, keepdim=True)


@functools.lru_cache(maxsize=None)
def oracle(n, L, B, G, kind):
    """(noise, gE, the float64 shift rule's rows) of a case; kind: mild | half | readme."""
    x, w, _ = inputs(n, L, B, G)
    noise = {"mild": mild_noise(n, L), "half": per_wire_noise(n), "readme": README_NOISE}[kind]
    gE = grad_out(n, B)
    return noise, gE, mixed_rows(x, w, gE, noise, "cpu").double()


def launch(x, w, gE, noise, want_E=True, fill=None):
    """The raw launcher on device tensors: (G, E or None)."""
    B, n = x.shape
    mk = (lambda *s: torch.empty(*s, device=x.device)) if fill is None else \
        (lambda *s: torch.full(s, fill, device=x.device))
    G, E = mk(B, 2 * n * w.shape[-3]), mk(B, n) if want_E else None
    Q.hip_qsim_mixed_adjoint(x, w, gE, G, E, noise, Q.wgroup_of(x, w))
    return G, E


def check(cuda, n, L, B, G, kind):
    x, w, _ = inputs(n, L, B, G)
    noise, gE, ref = oracle(n, L, B, G, kind)
    bd = bound(n, L, noise, gE)
    A = amplification(noise, n, L)
    if kind != "half":   # the conditions that keep the check from passing vacuously, on the host oracle
        assert A <= 4.0
        assert float(ref.abs().max(1).values.min()) > 10 * float(bd.max()), (float(ref.abs().max()), float(bd.max()))
    Gd, _ = launch(x.to(cuda), w.to(cuda), gE.to(cuda), noise, fill=SENTINEL)
    err = (Gd.cpu().double() - ref).abs()
    print(f"mixed adjoint {kind} n={n} L={L} B={B} G={G}: A = {A:.3g}, worst |dG| = {float(err.max()):.3e}, bound "
          f"{float(bd.min()):.3e} .. {float(bd.max()):.3e}, worst ratio {float((err / bd).max()):.4f}, max |G| = "
          f"{float(ref.abs().max()):.3e}")
    assert bool((Gd != SENTINEL).all())   # every column is written
    assert bool((err <= bd).all())
    assert torch.equal(mixed_adjoint_rows(x.to(cuda), w.to(cuda), gE.to(cuda), noise), Gd)   # the public function


# ------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("n,L,B,G", CASES)
def test_every_entry_against_the_shift_rule(cuda, n, L, B, G):
    check(cuda, n, L, B, G, "mild")


@pytest.mark.parametrize("n,L,B,G", CASES)
def test_rates_up_to_one_half(cuda, n, L, B, G):
    """0 and 0.5 among the rates of each kind: the same formula with this model's own amplification."""
    check(cuda, n, L, B, G, "half")


def test_readme_noise_point(cuda):
    check(cuda, *README_CASE, "readme")


@pytest.mark.parametrize("n,L,B", [(2, 1, 3), (4, 3, 2), (7, 2, 2), (8, 2, 2)])
def test_zero_noise_against_the_exact_kernel(cuda, n, L, B):
    """All rates zero: dx and the column sums against the state-vector adjoint (hip_qsim_bwd_slab).  That kernel's
    share: its probabilities are within n L 2^-17 in L1 after one pass (``exact_bound``) and its backward makes two
    more (the undo, lambda), then an fp32 sum: sum |gE| (3 n L 2^-17 + (2^n + 2) eps) per sample."""
    x, w, _ = inputs(n, L, B, 0)
    gE = grad_out(n, B)
    xd, wd, gd = x.to(cuda), w.to(cuda), gE.to(cuda)
    G = mixed_adjoint_rows(xd, wd, gd, NoiseModel())
    dx = torch.empty(B, n, device=cuda)
    slab = Q.hip_qsim_bwd_slab(xd, wd, gd, dx)
    bd = bound(n, L, NoiseModel(), gE) + gE.double().abs().sum(1, keepdim=True) * (2 * n * L * 2.0 ** -17 + exact_bound(n, L))
    e_dx = (G[:, 0:2 * n:2].cpu().double() - dx.cpu().double()).abs()
    e_dw = (G.cpu().double().sum(0) - slab.cpu().double().sum(0)).abs()
    print(f"zero noise n={n} L={L}: worst dx ratio {float((e_dx / bd).max()):.4f}, worst dw ratio "
          f"{float(e_dw.max() / float(bd.sum())):.4f}")
    assert bool((e_dx <= bd).all()) and bool((e_dw <= float(bd.sum())).all())
    assert float(dx.abs().max()) > 10 * float(bd.max())


# ------------------------------------------------------------------------------- exact relations
@pytest.mark.parametrize("n,L,B,G", CASES)
def test_e_out_is_the_forward_kernels(cuda, n, L, B, G):
    x, w, _ = inputs(n, L, B, G)
    for kind in ("mild", "half"):
        noise, gE, _ = oracle(n, L, B, G, kind)
        xd, wd = x.to(cuda), w.to(cuda)
        Gd, E = launch(xd, wd, gE.to(cuda), noise)
        E0 = torch.empty(B, n, device=cuda)
        Q.hip_qsim_mixed_fwd(xd, wd, E0, None, noise, Q.wgroup_of(xd, wd))
        assert torch.equal(E, E0)
        G2, none = launch(xd, wd, gE.to(cuda), noise, want_E=False)   # E_out = null: the same rows
        assert none is None and torch.equal(G2, Gd)


@pytest.mark.parametrize("n,L", [(6, 2), (7, 2), (8, 2)])
def test_a_row_alone_in_a_batch_and_in_a_reused_slot(cuda, n, L):
    """B = 3: each row alone, in the batch, and under a forced grid of 1 (every sample through slot 0)."""
    x, w, _ = inputs(n, L, 3, 0)
    noise, gE = per_wire_noise(n), grad_out(n, 3)
    xd, wd, gd = x.to(cuda), w.to(cuda), gE.to(cuda)
    G, E = launch(xd, wd, gd, noise)
    for b in range(3):
        G1, E1 = launch(xd[b:b + 1].contiguous(), wd, gd[b:b + 1].contiguous(), noise)
        assert torch.equal(G1[0], G[b]) and torch.equal(E1[0], E[b])
    try:
        Q.mixed_force_grid(1)
        G2, E2 = launch(xd, wd, gd, noise)
        torch.cuda.synchronize()
    finally:
        Q.mixed_force_grid(0)
    assert torch.equal(G2, G) and torch.equal(E2, E)


def test_grouped_weights_are_the_per_group_calls(cuda):
    n, L, B, G0 = 6, 2, 3, 3
    x, w, _ = inputs(n, L, B, G0)
    noise, gE = per_wire_noise(n), grad_out(n, B)
    xd, wd, gd = x.to(cuda), w.to(cuda), gE.to(cuda)
    G, _ = launch(xd, wd, gd, noise)
    for g in range(G0):
        Gg, _ = launch(xd[g:g + 1].contiguous(), wd[g].contiguous(), gd[g:g + 1].contiguous(), noise)
        assert torch.equal(Gg[0], G[g])
    assert not torch.equal(launch(xd, wd[0].contiguous(), gd, noise)[0][1:], G[1:])   # (the groups differ)


@pytest.mark.parametrize("n,L,B", [(5, 2, 3), (7, 2, 2), (8, 2, 2)])
def test_graph_replays_equal_eager(cuda, n, L, B):
    _, w, _ = inputs(n, L, B, 0)
    noise, gE = per_wire_noise(n), grad_out(n, B).to(cuda)
    xs = [torch.rand(B, n, generator=torch.Generator().manual_seed(s)) * 2 - 1 for s in (1, 2, 3)]
    wd = w.to(cuda)
    eager = [launch(xi.to(cuda), wd, gE, noise) for xi in xs]   # (also the warm-up: LDS opted in, thresholds uploaded)
    torch.cuda.synchronize()
    x = torch.zeros(B, n, device=cuda)
    G, E = torch.empty(B, 2 * n * L, device=cuda), torch.empty(B, n, device=cuda)
    ws = Q.mixed_adjoint_workspace(n, B, cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.hip_qsim_mixed_adjoint(x, wd, gE, G, E, noise, 0, ws)
    for xi, (Ge, Ee) in zip(xs, eager):
        x.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(G, Ge) and torch.equal(E, Ee)


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32)
@pytest.mark.parametrize("n,L,B", [(3, 2, 5), (6, 2, 3), (7, 2, 2), (8, 2, 3)])
def test_lds_poison(cuda, n, L, B, pattern):
    x, w, _ = inputs(n, L, B, 0)
    noise, gE = per_wire_noise(n), grad_out(n, B)
    xd, wd, gd = x.to(cuda), w.to(cuda), gE.to(cuda)
    clean = launch(xd, wd, gd, noise)
    try:
        nat.set_lds_poison(pattern)
        poisoned = launch(xd, wd, gd, noise)
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    assert torch.equal(clean[0], poisoned[0]) and torch.equal(clean[1], poisoned[1])
    assert bool(torch.isfinite(clean[0]).all())


def test_autograd_is_the_rows(cuda):
    n, L, B, G0 = 6, 2, 3, 3
    x, w, _ = inputs(n, L, B, G0)
    noise, gE = per_wire_noise(n), grad_out(n, B).to(cuda)
    xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
    E = qsim_mixed(xa, wa, noise, diff_method="adjoint")
    (E * gE).sum().backward()
    G = mixed_adjoint_rows(x.to(cuda), w.to(cuda), gE, noise)
    dx, dw = Q._rows_to_grads(G, x.to(cuda), w.to(cuda), "hip")
    assert torch.equal(E.detach(), qsim_mixed(x.to(cuda), w.to(cuda), noise))
    assert torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw)


# ------------------------------------------------------------------------------- the raw entry point
def test_entry_point_refusals(cuda):
    lib = nat.hip_lib()
    adj = nat.fn(lib, "qd_qsim_mixed_adjoint", [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
    wsb = nat.fn(lib, "qd_qsim_mixed_adjoint_workspace", [_i, _i], ctypes.c_longlong)
    assert wsb(6, 100) == 0 and wsb(7, 1) == 16 << 14 and wsb(8, 3) == 3 * (16 << 16) and wsb(9, 3) == 0
    assert wsb(8, 100000) == wsb(8, 50000) and wsb(7, 100000) == wsb(7, 50000)   # sized by the grid, not by B
    try:
        Q.mixed_force_grid(2)
        assert wsb(8, 100) == 2 * (16 << 16)
    finally:
        Q.mixed_force_grid(0)
    B = 2
    st = nat.stream_ptr(cuda)
    thr = NoiseModel(0.1, 0.1, 0.1, 0.1)
    ws = torch.empty(wsb(8, B), dtype=torch.uint8, device=cuda)

    def call(n, L, rows=B, wgroup=0, ws=None, null=None):
        x, w = torch.zeros(B, n, device=cuda), torch.zeros(max(L, 1), n, 2, device=cuda)
        t1, t2, tro = thr.thresholds(max(n, 2), cuda)
        gE = torch.ones(B, n, device=cuda)
        G = torch.full((B, 2 * n * max(L, 1)), SENTINEL, device=cuda)
        E = torch.full((B, n), SENTINEL, device=cuda)
        args = [nat.ptr(x), nat.ptr(w), nat.ptr(t1), nat.ptr(t2), nat.ptr(tro), nat.ptr(gE), nat.ptr(G), nat.ptr(E)]
        if null is not None:
            args[null] = None
        r = adj(*args, rows, n, L, wgroup, nat.ptr(ws) if ws is not None else None, st)
        torch.cuda.synchronize()
        return r, bool((G == SENTINEL).all()) and bool((E == SENTINEL).all())

    assert call(1, 1) == (INVALID, True)
    assert call(9, 1) == (INVALID, True)
    assert call(4, 0) == (INVALID, True)
    assert call(7, 1) == (INVALID, True) and call(8, 1) == (INVALID, True)   # n = 7, 8 without a workspace
    assert call(2, 1025) == (INVALID, True)         # 2 n L > 4096
    assert call(4, 1, rows=0) == (INVALID, True)
    assert call(4, 1, wgroup=3) == (INVALID, True)   # the groups do not divide the batch
    assert call(4, 1, wgroup=-1) == (INVALID, True)
    for null in (0, 1, 2, 3, 4, 5, 6):              # x, w, the thresholds, gE, G
        assert call(4, 1, null=null) == (INVALID, True)
    assert call(4, 1) == (0, False) and call(8, 1, ws=ws) == (0, False)
    # the Python functions refuse before any launch: a rate above 0.5, a short workspace
    x, w, gE = torch.zeros(2, 4, device=cuda), torch.zeros(1, 4, 2, device=cuda), torch.ones(2, 4, device=cuda)
    G = torch.full((2, 8), SENTINEL, device=cuda)
    for bad in (OverHalf(1, p1=0.1), OverHalf(2, p2=0.5)):
        with pytest.raises(ValueError, match="parameter_shift"):
            Q.hip_qsim_mixed_adjoint(x, w, gE, G, None, bad)
        with pytest.raises(ValueError, match="parameter_shift"):
            mixed_adjoint_rows(x, w, gE, bad)
        with pytest.raises(ValueError, match="parameter_shift"):
            qsim_mixed(x, w, bad, diff_method="adjoint")
        assert qsim_mixed(x, w, bad).shape == (2, 4)   # the shift rule's path takes them
    x8, w8 = torch.zeros(2, 8, device=cuda), torch.zeros(1, 8, 2, device=cuda)
    with pytest.raises(ValueError, match="workspace"):
        Q.hip_qsim_mixed_adjoint(x8, w8, torch.ones(2, 8, device=cuda), torch.empty(2, 16, device=cuda), None, thr, 0,
                                 torch.empty(16, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    assert bool((G == SENTINEL).all())


@pytest.mark.parametrize("n", [4, 8])
def test_kernel_guard_writes_nan_rows(cuda, n):
    """The entry point cannot read device thresholds before the launch; a workgroup that meets one above 2^31 takes no
    site's inverse and writes NaN rows (the Python launchers refuse on the host copies before that)."""
    L, B = 2, 2
    x, w, _ = inputs(n, L, B, 0)
    bad = OverHalf(1, p1=0.1)
    t1, t2, tro = bad.thresholds(n, cuda)
    xd, wd, gE = x.to(cuda), w.to(cuda), torch.ones(B, n, device=cuda)
    G = torch.full((B, 2 * n * L), SENTINEL, device=cuda)
    ws = Q.mixed_adjoint_workspace(n, B, cuda)
    adj = nat.fn(nat.hip_lib(), "qd_qsim_mixed_adjoint", [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
    r = adj(nat.ptr(xd), nat.ptr(wd), nat.ptr(t1), nat.ptr(t2), nat.ptr(tro), nat.ptr(gE), nat.ptr(G), None, B, n, L, 0,
            nat.ptr(ws) if ws is not None else None, nat.stream_ptr(cuda))
    torch.cuda.synchronize()
    assert r == 0 and bool(torch.isnan(G).all())


# ------------------------------------------------------------------------------- the fused step
STEP_NOISE = NoiseModel(0.05, 0.1, 0.03, 0.05)
STEP_SHAPES = [(4, 2, 18), (8, 3, 18)]


def build(device, n, L, B, groups=3):
    torch.manual_seed(0)
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=True, use_gradient_pruning=False, pilot_num=128,
                 noise_level=0.05).to(device).train()
    space = FlatParamSpace(list(m.named_parameters()), device)
    step = QSCStepHIP(m, space, B, n_groups=groups, noise=STEP_NOISE, exact_noise=True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 2, 16, 8, generator=g).to(device)
    y = torch.randint(0, 3, (B,), generator=g).to(device)
    return m, space, step, x, y


@pytest.mark.parametrize("n,L,B", STEP_SHAPES)
def test_fused_step_is_the_raw_launchers(cuda, n, L, B):
    m, space, step, x, y = build(cuda, n, L, B)
    assert step.measured and step.exact_noise and not hasattr(step, "shot_ctr")
    space.zero_grad()
    loss = step(x, y)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    angles, w, dE = step.angles.clone(), step._w_cur.clone(), step.dE.clone()
    assert w.dim() == 4 and w.shape[0] == 3   # the QuantumNAT streams' weights
    E = torch.empty_like(step.E)
    Q.hip_qsim_mixed_fwd(angles, w, E, None, STEP_NOISE, Q.wgroup_of(angles, w))
    assert torch.equal(step.E, E)
    G, _ = launch(angles, w, dE, STEP_NOISE, want_E=False)
    assert torch.equal(step.dang, G[:, 0:2 * n:2]) and torch.equal(step.Grows, G)
    gw = m.qlayer.weights.grad.detach().reshape(-1)
    want = G.double().sum(0)
    bd = (B + step.qrows) * 2.0 ** -23 * G.double().abs().sum(0)   # (the measured-step test's summation bound)
    err = (gw.double() - want).abs()
    print(f"exact-noise step n={n}: weight-gradient max error {float(err.max()):.3e}, smallest bound "
          f"{float(bd.min()):.3e}, max |grad| {float(gw.abs().max()):.3e}")
    assert step.qrows == -(-B // 64) and bool((err <= bd).all()) and float(gw.abs().max()) > 0


def test_fused_validation_is_the_exact_channel(cuda):
    """``ClassifierStep.forward`` in eval mode (the runner's validation) on an exact-noise step: per chunk of the
    step's batch, the last one padded, the density matrix on the step's angles and master weights, then the head.
    E is the raw launcher's bit for bit; the log-probabilities against an fp64 head on that E within 1e-5 (the fp32
    head's share, tests/test_mixed_gpu.py); the noiseless validation is more than ten times that away."""
    n, L, B, N = 4, 2, 18, 25
    m, space, step, _, _ = build(cuda, n, L, B)
    cstep = ClassifierStep(m, 3, space=space, batch_total=B, hip_kw=dict(noise=STEP_NOISE, exact_noise=True))
    h = cstep.hip
    assert h is not None and h.exact_noise
    m.eval()
    x = torch.randn(N, 2, 16, 8, generator=torch.Generator().manual_seed(9)).to(cuda)
    logp = cstep.forward(x)
    torch.cuda.synchronize()
    w = m.qlayer.weights.detach()
    W, b = m.classifier.weight.detach().cpu().double(), m.classifier.bias.detach().cpu().double()
    want, plain = [], []
    lp = torch.empty(B, 3, device=cuda)
    for lo in range(0, N, B):
        k = min(B, N - lo)
        xin = torch.cat([x[lo:lo + k], x[lo + k - 1:lo + k].expand(B - k, 2, 16, 8)]).contiguous()
        h.infer(xin, None, lp)   # the noiseless validation, and the step's angles of this chunk
        plain.append(lp[:k].clone())
        E = torch.empty(B, n, device=cuda)
        Q.hip_qsim_mixed_fwd(h.angles, w, E, None, STEP_NOISE)
        h.infer(xin, None, lp, noise=STEP_NOISE, exact_noise=True)
        assert torch.equal(h.E, E)
        want.append(torch.log_softmax(E.cpu().double() @ W.T + b, dim=1)[:k])
    d = float((logp.cpu().double() - torch.cat(want)).abs().max())
    away = float((logp - torch.cat(plain)).abs().max())
    print(f"fused validation: max |log p - reference| = {d:.3e}; the noiseless validation is {away:.3e} away")
    assert logp.shape == (N, 3) and d <= 1e-5 and away > 1e-4


def _world(cuda, n, L, B):
    m, space, step, x, y = build(cuda, n, L, B)
    opt = make_optimizer(space, "adamw", 1e-2, weight_decay=0.01, prune_thr=0.0)

    def run():
        space.zero_grad()
        step(x, y)
        opt.step()

    return space, step, run, [space.flat, opt.step_t, opt.pruned, opt.m, opt.v, step.noise_ctr]


@pytest.mark.parametrize("n,L,B", STEP_SHAPES)
def test_graphed_step_is_the_eager_step(cuda, n, L, B):
    sp1, st1, run1, _ = _world(cuda, n, L, B)
    for _ in range(3):
        run1()
    torch.cuda.synchronize()
    sp2, st2, run2, state = _world(cuda, n, L, B)
    assert st2.noise_seed == st1.noise_seed
    graphed = GraphedStep(run2)
    idx = torch.zeros(1, dtype=torch.long, device=cuda)
    _capture_preserving(graphed, state, idx, idx.clone())
    for _ in range(3):
        graphed()
    torch.cuda.synchronize()
    graphed.close()
    assert torch.equal(sp1.flat, sp2.flat) and torch.equal(st1.E, st2.E) and torch.equal(st1.Grows, st2.Grows)


def test_constructor_checks(cuda):
    def make(n=4, L=2, **kw):
        m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False).to(cuda)
        return QSCStepHIP(m, FlatParamSpace(list(m.named_parameters()), cuda), 6, **kw)

    assert make(noise=STEP_NOISE, exact_noise=True).exact_noise and not make().exact_noise
    with pytest.raises(ValueError, match="no shots"):
        make(noise=STEP_NOISE, exact_noise=True, shots=64)
    with pytest.raises(ValueError, match="adjoint"):
        make(noise=STEP_NOISE, exact_noise=True, diff_method="parameter_shift")
    with pytest.raises(ValueError, match="NoiseModel"):
        make(exact_noise=True)
    with pytest.raises(ValueError, match="mfma"):
        make(noise=STEP_NOISE, exact_noise=True, impl="ref")
    with pytest.raises(ValueError, match="n <= 8"):
        make(n=10, L=1, noise=STEP_NOISE, exact_noise=True)
    with pytest.raises(ValueError, match="parameter_shift"):
        make(noise=OverHalf(1, p1=0.1), exact_noise=True)
    with pytest.raises(ValueError, match="noise needs shots"):   # without the flag the old refusal stands
        make(noise=STEP_NOISE)


@pytest.mark.parametrize("where", ["fused", "module"])
def test_runner_trains_against_the_exact_channel(cuda, tmp_path, monkeypatch, where):
    made, replays, infers = [], [], []
    init, call, infer = ClassifierStep.__init__, GraphedStep.__call__, QSCStepHIP.infer

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    def spy_call(self, *a, **k):
        replays.append(self.graph is not None)
        return call(self, *a, **k)

    def spy_infer(self, *a, **k):
        infers.append((k.get("noise"), k.get("exact_noise", False)))
        return infer(self, *a, **k)

    monkeypatch.setattr(ClassifierStep, "__init__", spy_init)
    monkeypatch.setattr(GraphedStep, "__call__", spy_call)
    monkeypatch.setattr(QSCStepHIP, "infer", spy_infer)
    r = Y2HRunner(n_epochs=1, data_len=60, batch_size_DML=16, device="cuda", workspace=str(tmp_path / where),
                  data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2, use_quantumnat=True, seed=0,
                  qsc_noise_p1=0.02, qsc_noise_p2=0.05, qsc_readout01=0.02, qsc_readout10=0.03, qsc_noise_exact=True,
                  qsc_step=where)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = r.train_QSC_P128()
    h = made[-1].hip
    if where == "fused":
        assert h is not None and h.exact_noise and h.measured and h.shots is None
        assert replays and all(replays)   # the full batches ran as graph replays
        # validation ran on the step's kernels, every chunk under the training channel
        assert infers and all(nz is h.noise and ex is True for nz, ex in infers)
    else:
        assert h is None
    assert m.qlayer.exact_noise is True and m.qlayer.exact_diff_method == "adjoint"
    assert len(r.train_QSC_losses) == 1 and math.isfinite(r.train_QSC_losses[0]) and math.isfinite(r.val_QSC_losses[0])
    assert float(m.qlayer.weights.grad.abs().max()) > 0
