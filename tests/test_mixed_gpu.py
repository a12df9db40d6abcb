"""The density-matrix kernel (csrc/hip/qsim_mixed.hip; ops/quantum.py ``qsim_mixed`` / ``qsim_mixed_probs`` /
``mixed_rows`` on ``hip``): every element of E and of the probabilities against the float64 oracle within a derived
bound, the exact relations (batch, grid and slot independence, grouped weights, the readout's fma, graph replay, LDS
poisoning), zero noise against the exact kernel, the trajectory sampler's convergence to it, the gradients, the
inference engine's ``exact_noise`` and the raw entry point's refusals.

The bound (``bounds``), derived, not tuned.  eps = 2^-24; tau = 2^-21.4, ``__sincosf``'s absolute error (the project's
figure, tests/test_shots_stream_gpu.py).  The circuit is 2 n L sweeps over rho, n L of each kind:
  * a rotation sweep applies U = RZ.RY to the row bit and conj(U) to the column bit, then the one-qubit site.  The
    four trig values of U are each off by tau, so ||dU||_2 <= 3.5 tau, and d(U rho U^+) <= 2 ||dU||_2 ||rho|| = 7 tau
    both in the trace norm (||rho||_1 = 1) and in the Frobenius norm (||rho||_F <= 1).  Round-off: each of the two
    applications is a real rotation and a complex product per entry, the site three more operations, every rounding
    relative to terms bounded by the quad's entries -- at most 32 eps ||rho||_F <= 2^-19 in the Frobenius norm;
  * a CNOT sweep permutes exactly; its site sums a trace (<= 1) and mixes: at most 8 eps ||rho||_F <= 2^-21.
  Everything after a sweep is unitary conjugation and mixtures of it (the Pauli channels), which contract both norms,
  so the sweeps' errors add:  F = n L (7 tau + 2^-19 + 2^-21) in the Frobenius norm, and in the trace norm, where a
  round-off term of Frobenius size f may reach 2^(n/2) f,  T1 = n L (7 tau + 2^(n/2) (2^-19 + 2^-21)).
  * probabilities: |d rho_kk| <= F.
  * E_i = fma(c_i, S_i, d_i), S_i = tr(Z_i rho): |dS_i| <= ||Z_i|| T1 = T1, plus docs/PARITY.md's (K + 2) eps for the
    fp32 sum of K = 2^n terms of total size 1, plus the fma's eps:  |dE_i| <= |c_i| (T1 + (2^n + 2) eps) + eps."""
import ctypes
import fractions
import functools
import math

import numpy as np
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                               QSC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, mixed_readout,
                                                                                         mixed_rows, qsim, qsim_mixed,
                                                                                         qsim_mixed_probs, z_signs)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference
from test_noise_cpu import SEED, inputs as noise_inputs

pytestmark = pytest.mark.gpu

# (n, L, B, weight groups): rho below the workgroup size, odd sizes, more sweeps than one trig table holds at (4, 3),
# the largest LDS state (7: 128 KiB), the workspace path (8); one case with grouped weights
CASES = [(2, 1, 3, 0), (3, 2, 5, 0), (4, 3, 2, 0), (6, 2, 3, 3), (7, 2, 2, 0), (8, 3, 2, 0)]
SENTINEL = -7.0
INVALID = 1   # hipErrorInvalidValue
EPS, TAU = 2.0 ** -24, 2.0 ** -21.4
_p, _i = ctypes.c_void_p, ctypes.c_int


def bounds(n, L, c=1.0):
    """(per probability, per E_i with readout slope c): the module docstring's F and |c| (T1 + (2^n + 2) eps) + eps."""
    rnd = 2.0 ** -19 + 2.0 ** -21
    F = n * L * (7 * TAU + rnd)
    T1 = n * L * (7 * TAU + 2.0 ** (n / 2) * rnd)
    return F, abs(c) * (T1 + ((1 << n) + 2) * EPS) + EPS


def exact_bound(n, L):
    """The exact kernel's E (tests/test_shots_stream_gpu.py): the L1 error of its probabilities, n L 2^-17, plus the
    fp32 sum."""
    return n * L * 2.0 ** -17 + ((1 << n) + 2) * EPS


def per_wire_noise(n):
    """As tests/test_mixed_cpu.py: unequal rates per wire, 0 and 0.5 among the gate rates."""
    return NoiseModel(p1=np.linspace(0.0, 0.5, n), p2=np.linspace(0.5, 0.0, n), readout01=np.linspace(0.0, 0.1, n),
                      readout10=np.linspace(0.5, 0.05, n))


@functools.lru_cache(maxsize=None)
def case(n, L, B, G):
    """Host inputs (fp32) and the noise model."""
    g = torch.Generator().manual_seed(1000 * n + 10 * L + B)
    x = torch.rand(B, n, generator=g) * 2 - 1
    w = torch.rand(*((G,) if G else ()), L, n, 2, generator=g) * 2 * math.pi
    return x, w, per_wire_noise(n)


@functools.lru_cache(maxsize=None)
def oracle(n, L, B, G):
    """The float64 oracle's probabilities and E of ``case``."""
    x, w, noise = case(n, L, B, G)
    p = qsim_mixed_probs(x, w, noise, "cpu")
    c, d = mixed_readout(noise, n)
    return p, c * (p @ z_signs(n, dtype=torch.float64)) + d


def launch(x, w, noise, probs=True, fill=None):
    """The raw launcher on device tensors: (E, probs or None)."""
    B, n = x.shape
    mk = (lambda *s: torch.empty(*s, device=x.device)) if fill is None else \
        (lambda *s: torch.full(s, fill, device=x.device))
    E, p = mk(B, n), mk(B, 1 << n) if probs else None
    Q.hip_qsim_mixed_fwd(x, w, E, p, noise, Q.wgroup_of(x, w))
    return E, p


def fma32(c, s, d):
    """fl32(c s + d) of fp32 arrays, exactly: the rational value, then the nearest float (the double's float, or a
    neighbour of it)."""
    out = np.empty(s.shape, dtype=np.float32)
    for idx in np.ndindex(*s.shape):
        r = fractions.Fraction(float(c[idx[-1]])) * fractions.Fraction(float(s[idx])) + fractions.Fraction(float(d[idx[-1]]))
        f = np.float32(float(r))
        cand = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
        out[idx] = min(cand, key=lambda v: abs(fractions.Fraction(float(v)) - r))
    return out


# ------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("n,L,B,G", CASES)
def test_every_element_against_the_oracle(cuda, n, L, B, G):
    x, w, noise = case(n, L, B, G)
    p64, E64 = oracle(n, L, B, G)
    E, p = launch(x.to(cuda), w.to(cuda), noise, fill=SENTINEL)
    c, _ = mixed_readout(noise, n)
    bp = bounds(n, L)[0]
    bE = torch.tensor([bounds(n, L, float(ci))[1] for ci in c], dtype=torch.float64)
    ep = (p.cpu().double() - p64).abs()
    eE = (E.cpu().double() - E64).abs()
    print(f"mixed n={n} L={L} B={B} G={G}: probs worst |d| = {float(ep.max()):.3e}, bound {bp:.3e}, ratio "
          f"{float(ep.max()) / bp:.4f}; E worst |d| / bound = {float((eE / bE).max()):.4f} (bounds {float(bE.min()):.3e} "
          f".. {float(bE.max()):.3e})")
    assert bool((ep <= bp).all()) and bool((eE <= bE).all())
    ideal = qsim(x[:1], w[0] if G else w, "cpu")[0].double()
    assert float((E64[0] - ideal).abs().max()) > 10 * float(bE.max())   # the noiseless circuit fails the check
    # the public functions are these launches
    assert torch.equal(qsim_mixed_probs(x.to(cuda), w.to(cuda), noise), p)
    assert torch.equal(qsim_mixed(x.to(cuda), w.to(cuda), noise), E)


# ------------------------------------------------------------------------------- exact relations
@pytest.mark.parametrize("n,L,B,G", [(3, 2, 5, 0), (7, 2, 2, 0), (8, 3, 2, 0)])
def test_a_row_does_not_depend_on_the_batch(cuda, n, L, B, G):
    x, w, noise = case(n, L, B, G)
    xd, wd = x.to(cuda), w.to(cuda)
    E, p = launch(xd, wd, noise)
    for b in range(B):
        E1, p1 = launch(xd[b:b + 1].contiguous(), wd, noise)
        assert torch.equal(E1[0], E[b]) and torch.equal(p1[0], p[b])
    E2, none = launch(xd, wd, noise, probs=False)   # probs=None: the same E
    assert none is None and torch.equal(E2, E)


@pytest.mark.parametrize("n,L", [(8, 2), (5, 2)])
def test_forced_grid_reuses_slots(cuda, n, L):
    """Grid 2 at B = 5: three samples through slot 0, two through slot 1 -- the unforced run's bits."""
    x, w, noise = case(n, L, 5, 0)
    xd, wd = x.to(cuda), w.to(cuda)
    E, p = launch(xd, wd, noise)
    try:
        Q.mixed_force_grid(2)
        E2, p2 = launch(xd, wd, noise)
        torch.cuda.synchronize()
    finally:
        Q.mixed_force_grid(0)
    assert torch.equal(E2, E) and torch.equal(p2, p)


def test_grouped_weights_are_the_per_group_calls(cuda):
    n, L, B, G = 6, 2, 3, 3
    x, w, noise = case(n, L, B, G)
    xd, wd = x.to(cuda), w.to(cuda)
    E, p = launch(xd, wd, noise)
    for g in range(G):
        Eg, pg = launch(xd[g:g + 1].contiguous(), wd[g].contiguous(), noise)
        assert torch.equal(Eg[0], E[g]) and torch.equal(pg[0], p[g])
    assert not torch.equal(launch(xd, wd[0].contiguous(), noise)[0][1:], E[1:])   # (the groups differ)


@pytest.mark.parametrize("n,L", [(4, 2), (8, 2)])
def test_readout_alone_is_one_fma(cuda, n, L):
    x, w, _ = case(n, L, 2, 0)
    xd, wd = x.to(cuda), w.to(cuda)
    ro = NoiseModel(readout01=np.linspace(0.0, 0.1, n), readout10=np.linspace(0.5, 0.05, n))
    E0, p0 = launch(xd, wd, NoiseModel())
    E1, p1 = launch(xd, wd, ro)
    c, d = mixed_readout(ro, n)
    assert torch.equal(p1, p0)
    want = fma32(c.float().numpy(), E0.cpu().numpy(), d.float().numpy())
    assert c.float().double().equal(c) and d.float().double().equal(d)   # (the constants are exact in fp32)
    assert torch.equal(E1.cpu(), torch.from_numpy(want)) and not torch.equal(E1, E0)


@pytest.mark.parametrize("n,L,B", [(5, 2, 3), (8, 2, 2)])
def test_graph_replays_equal_eager(cuda, n, L, B):
    _, w, noise = case(n, L, B, 0)
    xs = [torch.rand(B, n, generator=torch.Generator().manual_seed(s)) * 2 - 1 for s in (1, 2)]
    wd = w.to(cuda)
    eager = [launch(xi.to(cuda), wd, noise) for xi in xs]   # (also the warm-up: launcher declared, LDS opted in)
    torch.cuda.synchronize()
    x = torch.zeros(B, n, device=cuda)
    E, p = torch.empty(B, n, device=cuda), torch.empty(B, 1 << n, device=cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.hip_qsim_mixed_fwd(x, wd, E, p, noise)
    for xi, (Ee, pe) in zip(xs, eager):
        x.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(E, Ee) and torch.equal(p, pe)


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32)
@pytest.mark.parametrize("n,L,B", [(3, 2, 5), (7, 2, 2), (8, 2, 5)])
def test_lds_poison(cuda, n, L, B, pattern):
    x, w, noise = case(n, L, B, 0)
    xd, wd = x.to(cuda), w.to(cuda)
    clean = launch(xd, wd, noise)
    try:
        nat.set_lds_poison(pattern)
        poisoned = launch(xd, wd, noise)
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    assert torch.equal(clean[0], poisoned[0]) and torch.equal(clean[1], poisoned[1])
    assert bool(torch.isfinite(clean[0]).all())


# ------------------------------------------------------------------------------- zero noise
@pytest.mark.parametrize("n,L,B", [(2, 1, 3), (5, 3, 3), (7, 2, 2), (8, 3, 2)])
def test_zero_noise_against_the_exact_kernel(cuda, n, L, B):
    x, w, _ = case(n, L, B, 0)
    xd, wd = x.to(cuda), w.to(cuda)
    d = (qsim_mixed(xd, wd, NoiseModel()).double() - qsim(xd, wd, "hip").double()).abs()
    bound = bounds(n, L)[1] + exact_bound(n, L)
    print(f"zero noise n={n} L={L}: worst |mixed - exact| = {float(d.max()):.3e}, bound {bound:.3e}")
    assert float(d.max()) <= bound


# ------------------------------------------------------------------------------- the samplers converge to it
def test_trajectory_sampler_converges_to_the_density_matrix(cuda):
    """tests/test_noise_cpu.py::test_channel_statistics_against_density_matrix with the kernels on both sides: the batch
    mean of B T trajectory means in [-1, 1] within 5 sigma = 5 / sqrt(B T) of the exact expectation."""
    n, L, B, shots, T = 3, 2, 64, 4096, 1024
    noise = NoiseModel(0.05, 0.1, 0.02, 0.05)
    x1, w = noise_inputs(n, L, 1)
    x = x1.expand(B, n).contiguous().to(cuda)
    wd = w.to(cuda)
    got = qsim(x, wd, "hip", shots=shots, seed=SEED, noise=noise, trajectories=T).double().mean(0).cpu()
    want = qsim_mixed(x1.to(cuda), wd, noise)[0].double().cpu()
    ideal = qsim(x1.to(cuda), wd, "hip")[0].double().cpu()
    bound = 5 / math.sqrt(B * T)
    print(f"sampled mean {got.tolist()}, density matrix {want.tolist()}, noiseless {ideal.tolist()}; bound {bound:.4f}; "
          f"max |got - dm| = {float((got - want).abs().max()):.4f}, max |ideal - dm| = "
          f"{float((ideal - want).abs().max()):.4f}")
    assert abs(bound - 0.0195) < 1e-4
    assert float((got - want).abs().max()) <= bound
    assert float((ideal - want).abs().max()) > bound   # the test cannot pass with the noise ignored


# ------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("n,L,B", [(3, 2, 4), (5, 2, 3), (8, 2, 1)])
def test_rows_against_the_cpu_rows(cuda, n, L, B):
    """Per entry sum_j |gE_j| times the forward bound of E_j (the rule's 1/2 times two evaluations); the reference's
    own fp32 result adds eps sum|gE|.  Milder rates than the forward cases' (which reach 0.5 and leave little
    gradient to check), still unequal per wire and with a 0."""
    x, w, _ = case(n, L, B, 0)
    noise = NoiseModel(p1=np.linspace(0.0, 0.05, n), p2=np.linspace(0.1, 0.0, n), readout01=np.linspace(0.0, 0.1, n),
                       readout10=np.linspace(0.2, 0.05, n))
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(3)) * 2 - 1
    ref = mixed_rows(x, w, gE, noise, "cpu").double()
    G = mixed_rows(x.to(cuda), w.to(cuda), gE.to(cuda), noise)
    assert G.shape == (B, 2 * n * L) and G.dtype == torch.float32
    c, _ = mixed_readout(noise, n)
    bE = torch.tensor([bounds(n, L, float(ci))[1] for ci in c], dtype=torch.float64)
    bound = (gE.double().abs() * (bE + EPS)).sum(1, keepdim=True)
    err = (G.cpu().double() - ref).abs()
    print(f"mixed rows n={n} L={L} B={B}: worst |dG| / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()) and float(ref.abs().max()) > 10 * float(bound.max())
    if n == 3:   # chunked over the parameters: the same bits
        budget = Q.MIXED_ROWS_BYTES
        try:
            Q.MIXED_ROWS_BYTES = 1
            assert torch.equal(mixed_rows(x.to(cuda), w.to(cuda), gE.to(cuda), noise), G)
        finally:
            Q.MIXED_ROWS_BYTES = budget
    # autograd: dx the layer-0 RY columns, dw the rows through reduce_slab
    xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
    (qsim_mixed(xa, wa, noise) * gE.to(cuda)).sum().backward()
    dw = Q.reduce_slab(G, torch.empty(2 * n * L, device=cuda)).view(L, n, 2)
    assert torch.equal(xa.grad, G[:, 0:2 * n:2]) and torch.equal(wa.grad, dw)


# ------------------------------------------------------------------------------- inference
N_INFER, CHUNK = 700, 576


@pytest.fixture(scope="module")
def engine(cuda):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(cuda).eval() for _ in range(3)]
    fc = FC_P128(128).to(cuda).eval()
    qsc = QSC_P128(8, 3, 3, False, False, 128).to(cuda).eval()
    x = torch.randn(N_INFER, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    return convs, fc, qsc, x


def test_inference_with_the_exact_channel(cuda, engine):
    convs, fc, qsc, x = engine
    noise = NoiseModel(p1=0.05, p2=0.1, readout01=0.02, readout10=0.2)
    eng = HIPInference(convs, fc, 128, cuda, chunk=CHUNK, qsc=qsc)
    with torch.no_grad():
        a, la = eng.classify(x, "quantum", noise=noise, exact_noise=True, return_logp=True)
        b = eng.classify(x, "quantum", noise=noise, exact_noise=True)
        plain, lplain = eng.classify(x, "quantum", return_logp=True)
        # the head's argmax over qsim_mixed on the engine's angles, chunk by chunk (the last one partial)
        preds = []
        for lo in range(0, x.shape[0], CHUNK):
            n = min(CHUNK, x.shape[0] - lo)
            eng._load(x, lo, n)
            eng.qsc.infer(eng.xq, eng.pred)
            E = qsim_mixed(eng.qsc.angles.detach().clone(), qsc.qlayer.weights.detach(), noise)
            logp = torch.log_softmax(E.cpu().double() @ qsc.classifier.weight.detach().cpu().double().T
                                     + qsc.classifier.bias.detach().cpu().double(), dim=1)[:n]
            top = logp.topk(2, dim=1).values
            preds.append((logp.argmax(1), top[:, 0] - top[:, 1], logp))
        small = HIPInference(convs, fc, 128, cuda, chunk=256, qsc=qsc).classify(x, "quantum", noise=noise,
                                                                                exact_noise=True)
    torch.cuda.synchronize()
    ref = torch.cat([p for p, _, _ in preds])
    keep = torch.cat([g for _, g, _ in preds]) > 1e-4   # (an fp32 head's near ties may fall either way)
    # the log-posterior: log_softmax moves by at most twice the largest logit error, a logit by its weight row's L1
    # norm times E's bound (the engine's E and the reference's are the same launches: this leaves the fp32 head, 1e-5)
    wl1 = float(qsc.classifier.weight.detach().abs().sum(1).max())
    tol = 2 * wl1 * bounds(8, 3)[1] + 1e-5
    dl = float((la.cpu().double() - torch.cat([l for _, _, l in preds])).abs().max())
    away = float((lplain.cpu().double() - la.cpu().double()).abs().max())
    print(f"log-posterior: max |engine - reference| = {dl:.3e} (tolerance {tol:.3e}); the noiseless one is {away:.3e} away")
    assert dl <= tol and away > 10 * tol   # the check fails with the noise ignored
    assert float(keep.float().mean()) >= 0.98
    assert torch.equal(a.cpu()[keep], ref[keep])
    assert torch.equal(a, b) and torch.equal(a, small)   # no Monte-Carlo: calls and chunk sizes agree
    assert torch.equal(la.argmax(1)[keep.to(cuda)], a[keep.to(cuda)])
    print(f"exact-noise prediction differs from the noiseless one on {float((a != plain).float().mean()):.4f}")
    with pytest.raises(ValueError, match="shots"):
        eng.classify(x, "quantum", noise=noise, exact_noise=True, shots=64)
    with pytest.raises(ValueError, match="NoiseModel"):
        eng.classify(x, "quantum", exact_noise=True)
    with pytest.raises(ValueError, match="quantum"):
        eng.classify(x, "classical", noise=noise, exact_noise=True)
    with pytest.raises(ValueError, match="noise needs shots"):   # without the flag the old refusal stands
        eng.classify(x, "quantum", noise=noise)
    with pytest.raises(ValueError, match="noise needs shots"):
        eng.qsc.infer(eng.xq, eng.pred, noise=noise)


# ------------------------------------------------------------------------------- the raw entry point
def test_entry_point_refusals(cuda):
    lib = nat.hip_lib()
    fwd = nat.fn(lib, "qd_qsim_mixed_fwd", [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
    ok = nat.fn(lib, "qd_qsim_mixed_ok", [_i, _i])
    wsb = nat.fn(lib, "qd_qsim_mixed_workspace", [_i, _i], ctypes.c_longlong)
    force = nat.fn(lib, "qd_qsim_mixed_force_grid", [_i])
    assert [ok(n, L) for n, L in ((1, 1), (2, 1), (8, 256), (8, 257), (9, 1), (4, 0), (2, 1024), (2, 1025))] == \
        [0, 1, 1, 0, 0, 0, 1, 0]
    assert wsb(7, 100) == 0 and wsb(8, 1) == 8 << 16 and wsb(8, 3) == 3 * (8 << 16) and wsb(9, 3) == 0
    assert wsb(8, 100000) == wsb(8, 50000)   # sized by the grid, not by B
    assert force(-1) == INVALID and force(2) == 0 and wsb(8, 100) == 2 * (8 << 16) and force(0) == 0
    B = 2
    st = nat.stream_ptr(cuda)
    thr = NoiseModel(0.1, 0.1, 0.1, 0.1)
    ws = torch.empty(wsb(8, B), dtype=torch.uint8, device=cuda)

    def call(n, L, rows=B, wgroup=0, ws=None, null=None):
        x, w = torch.zeros(B, n, device=cuda), torch.zeros(max(L, 1), n, 2, device=cuda)
        t1, t2, tro = thr.thresholds(max(n, 2), cuda)
        E = torch.full((B, n), SENTINEL, device=cuda)
        p = torch.full((B, 1 << n), SENTINEL, device=cuda)
        args = [nat.ptr(x), nat.ptr(w), nat.ptr(t1), nat.ptr(t2), nat.ptr(tro), nat.ptr(E), nat.ptr(p)]
        if null is not None:
            args[null] = None
        r = fwd(*args, rows, n, L, wgroup, nat.ptr(ws) if ws is not None else None, st)
        torch.cuda.synchronize()
        return r, bool((E == SENTINEL).all()) and bool((p == SENTINEL).all())

    assert call(1, 1) == (INVALID, True)
    assert call(9, 1) == (INVALID, True)
    assert call(4, 0) == (INVALID, True)
    assert call(8, 1) == (INVALID, True)            # n = 8 without a workspace
    assert call(2, 1025) == (INVALID, True)         # 2 n L > 4096
    assert call(4, 1, rows=0) == (INVALID, True)
    assert call(4, 1, wgroup=3) == (INVALID, True)   # the groups do not divide the batch
    assert call(4, 1, wgroup=-1) == (INVALID, True)
    for null in (0, 1, 2, 3, 4):
        assert call(4, 1, null=null) == (INVALID, True)
    assert call(4, 1) == (0, False) and call(8, 1, ws=ws) == (0, False)
    # the Python functions refuse before any launch
    x, w = torch.zeros(2, 9, device=cuda), torch.zeros(1, 9, 2, device=cuda)
    with pytest.raises(NotImplementedError, match="8"):
        qsim_mixed(x, w, thr)
    with pytest.raises(ValueError, match="CPU tensors"):
        qsim_mixed(x[:, :4].contiguous(), w[:, :4].contiguous(), thr, "cpu")
    with pytest.raises(ValueError, match="NoiseModel"):
        qsim_mixed(x[:, :4].contiguous(), w[:, :4].contiguous(), None)
