"""On-chip gradients on the HIP kernel (csrc/hip/qsim_onchip.hip): every shifted circuit's frames against the C++
oracle of the noise contract under the circuit's own counter, its probabilities against the framed fp64 oracle, its
expectations against the host's noisy sampler (bit for bit), G against its own expectations, zero rates against
qd_qsim_pshift, batch independence, the mask and need_dx, graph capture with a device counter, LDS poisoning, the
autograd and module paths and the entry point's range checks."""
import functools
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, counter_add,
                                                                                         noise_sites, pauli_frames,
                                                                                         pshift_counter, qsim,
                                                                                         qsim_probs, sample_z_noisy)

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32
NOISE = {"hi": NoiseModel(0.05, 0.1, 0.02, 0.03), "lo": NoiseModel(1e-3, 1e-2, 0.02, 0.03), "zero": NoiseModel()}
# (n, L, B, G, T, shots, rates): L = 1 with one trajectory and shots % 4 != 0, D below the block size, the timing
# point's rates, grouped weights, the largest LDS prefix, the register prefix
CASES = [(2, 1, 3, 0, 1, 65, "hi"), (5, 3, 3, 0, 4, 64, "hi"), (8, 3, 3, 0, 16, 256, "lo"),
         (8, 3, 6, 3, 16, 256, "hi"), (10, 2, 2, 0, 4, 64, "hi"), (12, 2, 2, 0, 4, 64, "hi")]
SENTINEL = -7


def atol_of(n):
    return 2e-5 if n <= 10 else 5e-5   # the project's tolerance of fp32 probabilities / expectations


@functools.lru_cache(maxsize=None)
def inputs(n, L, B, G):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if G == 0 else torch.rand(G, L, n, 2) * 2 * math.pi
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(2)) * 2 - 1
    return x, w, gE


@functools.lru_cache(maxsize=None)
def reference(n, L, B, G, T, rates):
    """The host oracle of every shifted circuit: frames (B, P, 2, T, L, 2) int32 drawn under the circuit's counter and
    the fp64 probabilities (B, P, 2, T, D) of the shifted circuit with those frames."""
    x, w, _ = inputs(n, L, B, G)
    P = 2 * n * L
    frames = torch.empty(B, P, 2, T, L, 2, dtype=torch.int32)
    probs = torch.empty(B, P, 2, T, 1 << n, dtype=torch.float64)
    xr = x.repeat_interleave(T, dim=0)
    for p in range(P):
        for s, sh in enumerate((0.5 * math.pi, -0.5 * math.pi)):
            F = pauli_frames(noise_sites(NOISE[rates], B, n, L, T, SEED_HI, pshift_counter(CTR_HI, p, s)))
            ws = w.clone()
            ws.view(-1, P)[:, p] += sh
            frames[:, p, s] = F
            probs[:, p, s] = qsim_probs(xr, ws, "cpu", frames=F.view(B * T, L, 2)).view(B, T, 1 << n)
    return frames, probs


def launch(x, w, gE, noise, T, shots, seed=SEED_HI, ctr0=CTR_HI, cptr=None, mask=None, need_dx=True, fill=None,
           want=True):
    """(G, Epm, probs, frames) of the raw launcher; ``fill``: the value the outputs hold before the launch."""
    B, n = x.shape
    L = w.shape[-3]
    P = 2 * n * L

    def mk(*s, dtype=torch.float32):
        if fill is None:
            return torch.empty(*s, device=x.device, dtype=dtype)
        return torch.full(s, fill, device=x.device, dtype=dtype)

    G = mk(B, P)
    Epm = mk(B, P, 2, n) if want else None
    probs = mk(B, P, 2, T, 1 << n) if want else None
    frames = mk(B, P, 2, T, L, 2, dtype=torch.int32) if want else None
    Q.hip_qsim_noisy_pshift(x, w, gE, G, Epm, probs, mask, need_dx, shots, seed, ctr0, cptr, Q.wgroup_of(x, w), noise, T,
                            frames)
    return G, Epm, probs, frames


def kinds_of(frames, n, L):
    """Counts of the four trajectory kinds over all circuits: no frame, a last-layer frame only, a frame before the
    circuit's shifted layer, a frame only at or after it (before the last layer)."""
    B, P = frames.shape[:2]
    nz = (frames != 0).any(-1)                                   # (B, P, 2, T, L)
    layer_of_p = (torch.arange(P) // (2 * n)).view(1, P, 1, 1, 1)
    m = torch.arange(L).view(1, 1, 1, 1, L)
    early = (nz & (m < layer_of_p) & (m < L - 1)).any(-1)
    late = (nz & (m >= layer_of_p) & (m < L - 1)).any(-1) & ~early
    inner = (nz & (m < L - 1)).any(-1)
    last_only = ~inner & nz[..., L - 1]
    none = ~nz.any(-1)
    return [int(t.sum()) for t in (none, last_only, early, late)]


@pytest.mark.parametrize("n,L,B,G,T,shots,rates", CASES)
def test_contract(cuda, n, L, B, G, T, shots, rates):
    x, w, gE = inputs(n, L, B, G)
    noise = NOISE[rates]
    fref, pref = reference(n, L, B, G, T, rates)
    P = 2 * n * L
    kinds = kinds_of(fref, n, L)
    print(f"n={n} L={L} B={B} G={G} T={T}: trajectory kinds none/last/early/late = {kinds} of {B * P * 2 * T}")
    if n >= 5:
        assert all(k > 0 for k in kinds), kinds   # every path of the kernel is exercised
    Gd, Epm, probs, frames = launch(x.to(cuda), w.to(cuda), gE.to(cuda), noise, T, shots)
    # 1. frames, exactly
    assert torch.equal(frames.cpu(), fref)
    # 2. probabilities against the framed fp64 oracle
    ep = float((probs.cpu().double() - pref).abs().max())
    print(f"  |dp| = {ep:.2e} (atol {atol_of(n):.0e})")
    assert ep <= atol_of(n)
    # 3. expectations: the host's noisy sampler on the kernel's own probabilities, no tolerance
    pc, fc = probs.cpu(), frames.cpu()
    for p in range(P):
        for s in range(2):
            ref = sample_z_noisy(pc[:, p, s], fc[:, p, s, :, L - 1, 0], noise, shots, SEED_HI,
                                 pshift_counter(CTR_HI, p, s))
            assert torch.equal(Epm[:, p, s].cpu(), ref), (p, s)
    # 4. the contraction: fp32 summation error only
    Ed, G64 = Epm.cpu().double(), Gd.cpu().double()
    sg = gE.double().abs().sum(1, keepdim=True)
    contr = (0.5 * (Ed[:, :, 0] - Ed[:, :, 1]) * gE.double()[:, None, :]).sum(-1)
    eG = float(((G64 - contr).abs() / sg).max())
    print(f"  |G - Epm.gE|/sum|gE| = {eG:.2e} (bound {n * 2.0 ** -23:.2e})")
    assert eG <= n * 2.0 ** -23
    # 6. a row's result does not depend on B
    one = launch(x[:1].to(cuda), (w if G == 0 else w[0]).to(cuda), gE[:1].to(cuda), noise, T, shots)
    for a, b in zip((Gd, Epm, probs, frames), one):
        assert torch.equal(a[:1], b)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("n,L,B", [(5, 3, 3), (8, 3, 3), (12, 2, 2)])
def test_zero_rates_are_the_pshift_kernel(cuda, n, L, B, T):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    shots = 64
    P = 2 * n * L
    Gd, Epm, probs, frames = launch(x, w, gE, NOISE["zero"], T, shots)
    G0 = torch.empty(B, P, device=cuda)
    E0 = torch.empty(B, P, 2, n, device=cuda)
    p0 = torch.empty(B, P, 2, 1 << n, device=cuda)
    Q.hip_qsim_pshift(x, w, gE, G0, E0, p0, None, True, shots, SEED_HI, CTR_HI)
    assert torch.equal(Gd, G0) and torch.equal(Epm, E0)
    assert torch.equal(probs, p0[:, :, :, None, :].expand_as(probs))
    assert not bool(frames.any())
    assert float(G0.abs().max()) > 0


@pytest.mark.parametrize("n,L,B,T", [(5, 3, 3, 4), (12, 2, 2, 4)])
def test_mask_and_need_dx(cuda, n, L, B, T):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    noise, shots = NOISE["hi"], 64
    full = launch(x, w, gE, noise, T, shots)
    mask = torch.rand(L, n, 2, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[0] = False           # all of layer 0
    mask[L - 1, 0] = True
    m8 = mask.reshape(-1).to(device=cuda, dtype=torch.uint8)
    ry0 = torch.zeros(L, n, 2, dtype=torch.bool)
    ry0[0, :, 0] = True
    for need_dx in (True, False):
        ran = (mask | ry0 if need_dx else mask).reshape(-1).to(cuda)
        assert bool(ran.any()) and not bool(ran.all())
        Gm, Em, pm, fm = launch(x, w, gE, noise, T, shots, mask=m8, need_dx=need_dx, fill=SENTINEL)
        assert torch.equal(Gm[:, ran], full[0][:, ran]) and torch.equal(Gm[:, ~ran], torch.zeros_like(Gm[:, ~ran]))
        for got, ref in zip((Em, pm, fm), full[1:]):
            assert torch.equal(got[:, ran], ref[:, ran])
            assert bool((got[:, ~ran] == SENTINEL).all())


def test_graph_capture_with_device_counter(cuda):
    n, L, B, T, shots = 8, 3, 3, 16, 256
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    noise = NOISE["lo"]
    eager = [launch(x, w, gE, noise, T, shots, ctr0=k, want=False)[0] for k in range(3)]
    ctr = torch.zeros((), dtype=torch.int64, device=cuda)
    G = torch.empty(B, 2 * n * L, device=cuda)
    kw = dict(shots=shots, seed=SEED_HI, counter_ptr=nat.ptr(ctr), noise=noise, trajectories=T)
    Q.hip_qsim_noisy_pshift(x, w, gE, G, **kw)   # (first launch outside)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Q.hip_qsim_noisy_pshift(x, w, gE, G, **kw)
        counter_add(ctr, 1)
    ctr.zero_()
    got = []
    for _ in range(3):
        g.replay()
        got.append(G.clone())
    torch.cuda.synchronize()
    assert int(ctr) == 3
    for k in range(3):
        assert torch.equal(got[k], eager[k]), k
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2]) and not torch.equal(got[0], got[2])


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32, the largest CDF word)
@pytest.mark.parametrize("n,L,B", [(5, 3, 3), (8, 3, 4), (12, 2, 2)])
def test_lds_poison(cuda, n, L, B, pattern):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, 0))
    runs = [("hi", 4, 64), ("zero", 1, 65)]
    clean = [launch(x, w, gE, NOISE[r], T, shots) for r, T, shots in runs]
    try:
        nat.set_lds_poison(pattern)
        poisoned = [launch(x, w, gE, NOISE[r], T, shots) for r, T, shots in runs]
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    for c, p in zip(clean, poisoned):
        for a, b in zip(c, p):
            assert torch.equal(a, b)


@pytest.mark.parametrize("n,L,B,G,T,shots", [(5, 3, 3, 0, 4, 64), (8, 3, 6, 3, 16, 256)])
def test_autograd(cuda, n, L, B, G, T, shots):
    x, w, gE = (t.to(cuda) for t in inputs(n, L, B, G))
    noise = NOISE["hi"]
    P = 2 * n * L
    Gd = launch(x, w, gE, noise, T, shots, want=False)[0]
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    E = qsim(xa, wa, "hip", shots=shots, seed=SEED_HI, counter=CTR_HI, diff_method="on_chip", noise=noise,
             trajectories=T)
    # the forward is the noisy forward (stream id 0)
    assert torch.equal(E, qsim(x, w, "hip", shots=shots, seed=SEED_HI, counter=CTR_HI, noise=noise, trajectories=T))
    (E * gE).sum().backward()
    assert torch.equal(xa.grad, Gd[:, 0:2 * n:2])
    dw = Q.reduce_slab(Gd, torch.empty(P, device=cuda))
    got = wa.grad if G == 0 else wa.grad[0]
    assert torch.equal(got.reshape(-1), dw)
    err = (dw.double() - Gd.double().sum(0)).abs()
    assert bool((err <= B * 2.0 ** -23 * Gd.double().abs().sum(0)).all())   # fp32 summation over the batch
    assert float(dw.abs().max()) > 0
    if G:
        assert float(wa.grad[1:].abs().max()) == 0   # the master gradient sits in group 0


def test_module_backward_is_the_kernel(cuda):
    torch.manual_seed(0)
    n, L, B, T, shots = 8, 3, 6, 16, 256
    noise = NOISE["lo"]
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False, shots=shots,
                 diff_method="on_chip", noise=noise, trajectories=T).to(cuda).train()
    m.qlayer.manual_shot_seed(SEED_HI)
    seen = {}

    def hook(_, inp, out):
        seen["angles"] = inp[0].detach().float().contiguous()
        out.register_hook(lambda g: seen.__setitem__("gE", g.detach().float().contiguous()))

    m.qlayer.register_forward_hook(hook)
    inp = torch.randn(B, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    torch.nn.functional.nll_loss(m(inp), torch.arange(B, device=cuda) % 3).backward()
    G = launch(seen["angles"], m.qlayer.weights.detach().contiguous(), seen["gE"], noise, T, shots, SEED_HI, 0,
               want=False)[0].double()
    err = (m.qlayer.weights.grad.reshape(-1).double() - G.sum(0)).abs()
    assert bool((err <= B * 2.0 ** -23 * G.abs().sum(0)).all())   # fp32 summation over the batch
    assert float(G.abs().max()) > 0 and m.preprocess[0].weight.grad is not None
    assert bool(torch.isfinite(m.preprocess[0].weight.grad).all())


def test_ungraphed_classifier_step_with_per_stream_weights(cuda):
    """ClassifierStep's module path draws QuantumNAT weight noise per stream (grouped w): it runs with on_chip."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep
    torch.manual_seed(0)
    n, L, S, B = 5, 2, 3, 2
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=True, use_gradient_pruning=False, shots=64,
                 diff_method="on_chip", noise=NOISE["hi"], trajectories=4).to(cuda).train()
    m.qlayer.shift_mask = torch.ones(L, n, 2, dtype=torch.bool)
    step = ClassifierStep(m, S)
    assert step.hip is None
    x = torch.randn(S * B, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    loss = step(x, torch.arange(S * B, device=cuda) % 3)
    g = m.qlayer.weights.grad
    assert math.isfinite(float(loss)) and g is not None and g.shape == (L, n, 2)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and float(step.skip) == 0


def test_range_checks(cuda):
    noise = NOISE["hi"]
    x, w = torch.zeros(2, 13, device=cuda), torch.zeros(1, 13, 2, device=cuda)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=64, diff_method="on_chip", noise=noise)
    # the entry point itself refuses what is out of range (hipErrorInvalidValue = 1), launching nothing
    f = nat.fn(nat.hip_lib(), "qd_qsim_noisy_pshift",
               [Q._p] * 11 + [Q._i] * 7 + [Q._u64, Q._u64, Q._p, Q._p])
    thr1, thr2, thr_ro = noise.thresholds(12, cuda)
    buf = torch.full((1 << 16,), float(SENTINEL), device=cuda)   # every pointer argument: nothing may be written

    def status(n, L, shots, T):
        return f(nat.ptr(buf), nat.ptr(buf), nat.ptr(buf), nat.ptr(buf), None, None, None, None, nat.ptr(thr1),
                 nat.ptr(thr2), nat.ptr(thr_ro), 1, n, L, 0, 1, shots, T, SEED_HI, CTR_HI, None, nat.stream_ptr(cuda))

    assert status(13, 1, 64, 1) == 1
    assert status(4, 2, 64, 3) == 1            # shots % T != 0
    assert status(4, 2, 60, 6) == 1            # T > 1 and (shots / T) % 4 != 0
    assert status(4, 2, 0, 1) == 1
    assert status(2, 8192, 64, 1) == 1         # 4 n L + 1 >= 2^16
    assert status(4, 513, 64, 1) == 1          # 2 n L > 4096 error sites
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    x, w, gE = torch.zeros(1, 2, device=cuda), torch.zeros(2, 2, 2, device=cuda), torch.zeros(1, 2, device=cuda)
    G = torch.empty(1, 8, device=cuda)
    with pytest.raises(RuntimeError, match="status 1"):
        Q.hip_qsim_noisy_pshift(x, w, gE, G, shots=64, noise=noise, trajectories=3)
