"""Noise-aware adjoint gradients on the HIP kernel (csrc/hip/qsim_nadj.hip): frames against the C++ oracle of the
noise contract (exactly), Ebar and G against the fp64 composition of the host oracles, zero thresholds against the
existing adjoint kernels and across T (bit for bit), the untouched forward, the autograd and module paths, graph
capture with a device counter, LDS poisoning and the entry point's range checks."""
import functools
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, counter_add,
                                                                                         noise_sites,
                                                                                         noisy_adjoint_rows,
                                                                                         pauli_frames, qsim)

pytestmark = pytest.mark.gpu

SEED, CTR = 7, 3
NOISE = {"hi": NoiseModel(0.05, 0.1, 0.03, 0.05), "lo": NoiseModel(1e-3, 1e-2, 0.02, 0.02), "zero": NoiseModel()}
# (n, L, B, T, groups): both sides of the 512-amplitude sweep variants, the n >= 10 trajectory split (T = 16: four
# chunks, T = 8: two, T = 4: none), two workgroups per CU at n = 12, L = 1 (a last-layer frame only), grouped weights
CASES = [(3, 2, 4, 8, 0), (5, 3, 3, 4, 0), (8, 3, 3, 16, 3), (9, 2, 3, 8, 0), (10, 3, 2, 16, 0), (11, 2, 2, 8, 0),
         (12, 3, 2, 16, 0), (12, 2, 2, 4, 0), (4, 1, 3, 4, 0)]
SENTINEL = -7.0


def atol_E(n):
    return 2e-5 if n <= 10 else 5e-5   # the project's tolerance of fp32 expectations (tests/test_onchip_gpu.py)


def atol_G(n):
    return 5e-5 if n <= 10 else 2e-4   # what tests/test_qsim12_gpu.py grants the adjoints' per-sample dx


@functools.lru_cache(maxsize=None)
def inputs(n, L, B, groups):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if groups == 0 else torch.rand(groups, L, n, 2) * 2 * math.pi
    gE = torch.randn(B, n, generator=torch.Generator().manual_seed(2))
    return x, w, gE


@functools.lru_cache(maxsize=None)
def reference(n, L, B, T, groups, rates):
    """(frames (B, T, L, 2) int32, G (B, 2nL) fp32 rounded from fp64, Ebar (B, n) fp64) of the host composition."""
    x, w, gE = inputs(n, L, B, groups)
    frames = pauli_frames(noise_sites(NOISE[rates], B, n, L, T, SEED, CTR))
    G, Ebar = noisy_adjoint_rows(x, w, gE, NOISE[rates], T, SEED, CTR, "cpu", return_expectation=True)
    return frames, G, Ebar


def launch(x, w, gE, noise, T, seed=SEED, ctr0=CTR, cptr=None, want=True):
    """(G, Ebar, frames) of the raw launcher."""
    B, n = x.shape
    L = w.shape[-3]
    G = torch.full((B, 2 * n * L), SENTINEL, device=x.device)
    Ebar = torch.full((B, n), SENTINEL, device=x.device) if want else None
    frames = torch.full((B, T, L, 2), -7, device=x.device, dtype=torch.int32) if want else None
    Q.hip_qsim_noisy_adjoint(x, w, gE, G, noise, T, seed, ctr0, cptr, Q.wgroup_of(x, w), Ebar, frames)
    return G, Ebar, frames


def reduce_slab(G):
    return Q.reduce_slab(G, torch.empty(G.shape[1], device=G.device))


@pytest.mark.parametrize("rates", ["hi", "lo"])
@pytest.mark.parametrize("n,L,B,T,groups", CASES)
def test_kernel_against_the_fp64_composition(cuda, n, L, B, T, groups, rates):
    x, w, gE = inputs(n, L, B, groups)
    fref, Gref, Eref = reference(n, L, B, T, groups, rates)
    # the host frames: which paths of the kernel this case takes
    rebuild = (fref[:, :, :L - 1] != 0).flatten(2).any(-1)          # (B, T)
    flips = fref[:, :, L - 1, 0] != 0
    per_row = rebuild.sum(1).tolist()
    print(f"n={n} L={L} B={B} T={T} {rates}: rebuilding trajectories per row {per_row}, "
          f"last X masks {int(flips.sum())}")
    if rates == "hi":
        assert L < 2 or bool(rebuild.any())
        assert bool(flips.any())
    Gd, Ed, Fd = launch(x.to(cuda), w.to(cuda), gE.to(cuda), NOISE[rates], T)
    assert torch.equal(Fd.cpu(), fref)
    eE = float((Ed.cpu().double() - Eref).abs().max())
    eG = float((Gd.cpu().double() - Gref.double()).abs().max())
    print(f"  |dEbar| = {eE:.2e} (atol {atol_E(n):.0e})   |dG| = {eG:.2e} (atol {atol_G(n):.0e}), "
          f"|G|max = {float(Gref.abs().max()):.3f}")
    assert eE <= atol_E(n)
    assert eG <= atol_G(n)
    assert float(Gref.abs().max()) > 1e-2
    # deterministic, and G does not depend on whether Ebar / frames are asked for
    again = launch(x.to(cuda), w.to(cuda), gE.to(cuda), NOISE[rates], T, want=False)[0]
    assert torch.equal(again, Gd)


@pytest.mark.parametrize("rates", ["hi", "lo"])
def test_deep_circuit(cuda, rates):
    """Forty layers: nearly every trajectory rebuilds at "hi", and a row is summed over 40 layers' passes.  The
    bounds are the shallow cases'."""
    n, L, B, T = 4, 40, 2, 4
    x, w, gE = inputs(n, L, B, 0)
    fref, Gref, Eref = reference(n, L, B, T, 0, rates)
    Gd, Ed, Fd = launch(x.to(cuda), w.to(cuda), gE.to(cuda), NOISE[rates], T)
    assert torch.equal(Fd.cpu(), fref)
    eE = float((Ed.cpu().double() - Eref).abs().max())
    eG = float((Gd.cpu().double() - Gref.double()).abs().max())
    print(f"n={n} L={L} {rates}: |dEbar| = {eE:.2e}, |dG| = {eG:.2e}, |G|max = {float(Gref.abs().max()):.3f}")
    assert eE <= atol_E(n) and eG <= atol_G(n)
    assert float(Gref.abs().max()) > 1e-2
    assert torch.equal(launch(x.to(cuda), w.to(cuda), gE.to(cuda), NOISE[rates], T, want=False)[0], Gd)


def test_some_row_mixes_both_kinds_of_trajectory():
    """The shared pass and the rebuild passes meet in one row's sum: from the host frames of the cases above."""
    mixed = []
    for n, L, B, T, groups in CASES:
        f = reference(n, L, B, T, groups, "hi")[0]
        r = (f[:, :, :L - 1] != 0).flatten(2).any(-1).sum(1)
        mixed.append(bool(((r > 0) & (r < T)).any()))
    print("cases with a mixed row:", mixed)
    assert any(mixed)


@pytest.mark.parametrize("n,L,B", [(5, 3, 3), (8, 3, 3), (10, 3, 2), (12, 2, 2)])
def test_zero_thresholds(cuda, n, L, B):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    runs = [launch(x, w, gE, NOISE["zero"], T) for T in (1, 4, 16)]
    for G, Ebar, frames in runs[1:]:
        assert torch.equal(G.view(torch.int32), runs[0][0].view(torch.int32))   # bit for bit, whatever T
        assert torch.equal(Ebar, runs[0][1]) and not bool(frames.any())
    G, Ebar, _ = runs[0]
    dx = torch.empty_like(x)
    slab = Q.hip_qsim_bwd_slab(x, w, gE, dx)
    E = torch.empty(B, n, device=cuda)
    Q.hip_qsim_fwd(x, w, E)
    edx = float((G[:, 0:2 * n:2] - dx).abs().max())
    edw = float((G.double().sum(0) - slab.double().sum(0)).abs().max())
    eE = float((Ebar - E).abs().max())
    print(f"n={n}: |dx - adjoint dx| = {edx:.2e}, |dw - adjoint dw| = {edw:.2e}, |Ebar - E| = {eE:.2e}")
    assert edx <= atol_G(n) and edw <= atol_G(n) and eE <= atol_E(n)
    assert float(dx.abs().max()) > 1e-2


@pytest.mark.parametrize("n,L,B,T,groups", [(5, 3, 3, 4, 0), (8, 3, 6, 16, 3), (10, 2, 2, 8, 0)])
def test_autograd_and_untouched_forward(cuda, n, L, B, T, groups):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, groups))
    noise, shots = NOISE["hi"], 256
    P = 2 * n * L
    Gd = launch(x, w, gE, noise, T, want=False)[0]
    kw = dict(shots=shots, seed=SEED, counter=CTR, noise=noise, trajectories=T)
    got = []
    for _ in range(2):
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        E = qsim(xa, wa, "hip", diff_method="noisy_adjoint", **kw)
        assert torch.equal(E, qsim(x, w, "hip", **kw))   # the forward of diff_method="adjoint", bit for bit
        (E * gE).sum().backward()
        got.append((xa.grad, wa.grad))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[0][0], Gd[:, 0:2 * n:2])
    dw = got[0][1] if groups == 0 else got[0][1][0]
    assert torch.equal(dw.reshape(-1), reduce_slab(Gd))
    err = (dw.reshape(-1).double() - Gd.double().sum(0)).abs()
    assert bool((err <= B * 2.0 ** -23 * Gd.double().abs().sum(0)).all())   # fp32 summation over the batch
    assert float(dw.abs().max()) > 0
    if groups:
        assert float(got[0][1][1:].abs().max()) == 0   # the master gradient sits in group 0


@pytest.mark.parametrize("n,L,B,T", [(8, 3, 3, 16), (10, 2, 2, 8)])
def test_graph_capture_with_device_counter(cuda, n, L, B, T):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    noise, shots = NOISE["hi"], 256
    eagerG, eagerE = [], []
    for k in range(3):
        eagerG.append(launch(x, w, gE, noise, T, ctr0=k, want=False)[0])
        E = torch.empty(B, n, device=cuda)
        Q.hip_qsim_noisy_shots_fwd(x, w, E, None, noise, shots, T, SEED, k)
        eagerE.append(E)
    ctr = torch.zeros((), dtype=torch.int64, device=cuda)
    G = torch.empty(B, 2 * n * L, device=cuda)
    E = torch.empty(B, n, device=cuda)

    def step():   # forward, backward, then the counter: the backward reads the value the forward read
        Q.hip_qsim_noisy_shots_fwd(x, w, E, None, noise, shots, T, SEED, 0, nat.ptr(ctr))
        Q.hip_qsim_noisy_adjoint(x, w, gE, G, noise, T, SEED, 0, nat.ptr(ctr))
        counter_add(ctr, 1)

    step()   # (first launch outside)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    ctr.zero_()
    got = []
    for _ in range(3):
        g.replay()
        got.append((G.clone(), E.clone()))
    torch.cuda.synchronize()
    assert int(ctr) == 3
    for k in range(3):
        assert torch.equal(got[k][0], eagerG[k]) and torch.equal(got[k][1], eagerE[k]), k
    assert not torch.equal(got[0][0], got[1][0]) and not torch.equal(got[1][0], got[2][0])


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32)
@pytest.mark.parametrize("n,L,B,T", [(5, 3, 3, 4), (12, 2, 2, 8)])
def test_lds_poison(cuda, n, L, B, T, pattern):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    clean = [launch(x, w, gE, NOISE[r], T) for r in ("hi", "zero")]
    try:
        nat.set_lds_poison(pattern)
        poisoned = [launch(x, w, gE, NOISE[r], T) for r in ("hi", "zero")]
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    for c, p in zip(clean, poisoned):
        for a, b in zip(c, p):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(c[0]).all())


def test_range_checks(cuda):
    noise = NOISE["hi"]
    x, w = torch.zeros(2, 13, device=cuda), torch.zeros(1, 13, 2, device=cuda)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=64, diff_method="noisy_adjoint", noise=noise)
    with pytest.raises(NotImplementedError, match="12"):
        noisy_adjoint_rows(x, w, torch.zeros(2, 13, device=cuda), noise)
    # the entry point itself refuses what is out of range (hipErrorInvalidValue = 1), launching nothing
    f = nat.fn(nat.hip_lib(), "qd_qsim_noisy_adjoint", [Q._p] * 10 + [Q._i] * 5 + [Q._u64, Q._u64, Q._p, Q._p])
    thr1, thr2, thr_ro = noise.thresholds(12, cuda)
    buf = torch.full((1 << 16,), SENTINEL, device=cuda)   # every pointer argument: nothing may be written

    def status(B, n, L, T, wgroup=0):
        return f(nat.ptr(buf), nat.ptr(buf), nat.ptr(buf), nat.ptr(buf), nat.ptr(buf), None, nat.ptr(buf),
                 nat.ptr(thr1), nat.ptr(thr2), nat.ptr(thr_ro), B, n, L, wgroup, T, SEED, CTR, None,
                 nat.stream_ptr(cuda))

    assert status(1, 13, 1, 1) == 1 and status(1, 1, 1, 1) == 1
    assert status(1, 4, 2, 0) == 1 and status(1, 4, 2, 1025) == 1
    assert status(1, 4, 513, 1) == 1           # 2 n L > 4096
    assert status(0, 4, 2, 1) == 1 and status(1, 4, 0, 1) == 1
    assert status(3, 4, 2, 1, wgroup=2) == 1   # wgroup does not divide B
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    x, w, gE = torch.zeros(1, 2, device=cuda), torch.zeros(2, 2, 2, device=cuda), torch.zeros(1, 2, device=cuda)
    G = torch.full((1, 8), SENTINEL, device=cuda)
    with pytest.raises(RuntimeError, match="status 1"):
        Q.hip_qsim_noisy_adjoint(x, w, gE, G, noise, 0)
    wl = torch.zeros(1025, 2, 2, device=cuda)
    Gl = torch.full((1, 4100), SENTINEL, device=cuda)
    with pytest.raises(RuntimeError, match="status 1"):
        Q.hip_qsim_noisy_adjoint(x, wl, gE, Gl, noise, 4)
    torch.cuda.synchronize()
    assert bool((G == SENTINEL).all()) and bool((Gl == SENTINEL).all())


def test_module_backward_reaches_the_cnn(cuda):
    torch.manual_seed(0)
    n, L, B, T, shots = 8, 3, 6, 16, 256
    noise = NOISE["hi"]
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False, shots=shots,
                 diff_method="noisy_adjoint", noise=noise, trajectories=T).to(cuda).train()
    m.qlayer.manual_shot_seed(SEED)
    seen = {}

    def hook(_, inp, out):
        seen["angles"] = inp[0].detach().float().contiguous()
        out.register_hook(lambda g: seen.__setitem__("gE", g.detach().float().contiguous()))

    m.qlayer.register_forward_hook(hook)
    inp = torch.randn(B, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    torch.nn.functional.nll_loss(m(inp), torch.arange(B, device=cuda) % 3).backward()
    G = launch(seen["angles"], m.qlayer.weights.detach().contiguous(), seen["gE"], noise, T, SEED, 0, want=False)[0]
    assert torch.equal(m.qlayer.weights.grad.reshape(-1), reduce_slab(G))
    g0 = m.preprocess[0].weight.grad
    assert g0 is not None and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0


def test_ungraphed_classifier_step_with_per_stream_weights(cuda):
    """ClassifierStep's module path draws QuantumNAT weight noise per stream (grouped w): it runs with noisy_adjoint."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep
    torch.manual_seed(0)
    n, L, S, B = 5, 2, 3, 2
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=True, use_gradient_pruning=False, shots=64,
                 diff_method="noisy_adjoint", noise=NOISE["hi"], trajectories=4).to(cuda).train()
    step = ClassifierStep(m, S)
    assert step.hip is None
    x = torch.randn(S * B, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    loss = step(x, torch.arange(S * B, device=cuda) % 3)
    g = m.qlayer.weights.grad
    assert math.isfinite(float(loss)) and g is not None and g.shape == (L, n, 2)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and float(step.skip) == 0
