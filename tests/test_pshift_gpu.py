"""Parameter-shift gradients on the HIP kernel (csrc/hip/qsim_pshift.hip): the shifted circuits' probabilities and
expectations against the fp64 oracle, the shot streams against the existing sampler (bit for bit), G against its own
expectations, the shot-noise bound, the mask and need_dx, graph capture with a device counter, LDS poisoning and the
module path."""
import functools
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (counter_add, pshift_counter,
                                                                                         qsim, qsim_probs, sample_z,
                                                                                         z_signs)

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32
# (n, L, B, G): L = 1, D below the block size, the register / LDS boundary of the exact simulators, the largest
# state, grouped weights (G, L, n, 2)
CASES = [(2, 1, 3, 0), (5, 3, 3, 0), (8, 3, 4, 0), (10, 2, 2, 0), (12, 2, 2, 0), (8, 3, 6, 3)]
SENTINEL = -7.0


def atol_of(n):
    return 2e-5 if n <= 10 else 5e-5   # the project's tolerance of fp32 probabilities / expectations


@functools.lru_cache(maxsize=None)
def case(n, L, B, G):
    """Host inputs and the fp64 reference of the 2P shifted circuits: probs (B, P, 2, D), E (B, P, 2, n), G_exact
    (B, P) and sigma1 (B, P), the standard deviation of G's one-shot-per-circuit estimate (sigma^2 = (Var+ + Var-) / 4,
    Var+- = p . v^2 - (p . v)^2, v = z_signs @ gE[b])."""
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if G == 0 else torch.rand(G, L, n, 2) * 2 * math.pi
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(2)) * 2 - 1
    P = 2 * n * L
    zs = z_signs(n, dtype=torch.float64)
    pr = torch.empty(B, P, 2, 1 << n, dtype=torch.float64)
    for p in range(P):
        for s, sh in enumerate((0.5 * math.pi, -0.5 * math.pi)):
            ws = w.clone()
            ws.view(-1, P)[:, p] += sh
            pr[:, p, s] = qsim_probs(x, ws, "cpu")
    E = pr @ zs
    v = (gE.double() @ zs.T)[:, None, None, :]
    mean = (pr * v).sum(-1)
    var = ((pr * v * v).sum(-1) - mean ** 2).clamp_min(0).sum(-1)
    return x, w, gE, pr, E, 0.5 * (mean[:, :, 0] - mean[:, :, 1]), (var / 4).sqrt()


def launch(x, w, gE, shots=0, seed=0, ctr0=0, cptr=None, mask=None, need_dx=True, fill=None, want=(True, True)):
    """(G, Epm, probs) of the raw launcher; ``fill``: the value the outputs hold before the launch."""
    B, n = x.shape
    P = 2 * n * w.shape[-3]
    mk = (lambda *s: torch.full(s, fill, device=x.device)) if fill is not None else \
        (lambda *s: torch.empty(*s, device=x.device))
    G = mk(B, P)
    Epm = mk(B, P, 2, n) if want[0] else None
    probs = mk(B, P, 2, 1 << n) if want[1] else None
    Q.hip_qsim_pshift(x, w, gE, G, Epm, probs, mask, need_dx, shots, seed, ctr0, cptr, Q.wgroup_of(x, w))
    return G, Epm, probs


@pytest.mark.parametrize("n,L,B,G", CASES)
def test_exact_mode(cuda, n, L, B, G):
    x, w, gE, pr, E, G_exact, _ = case(n, L, B, G)
    atol = atol_of(n)
    Gd, Epm, probs = launch(x.to(cuda), w.to(cuda), gE.to(cuda))
    sg = gE.double().abs().sum(1, keepdim=True)
    ep = float((probs.cpu().double() - pr).abs().max())
    eE = float((Epm.cpu().double() - E).abs().max())
    eG = float(((Gd.cpu().double() - G_exact).abs() / sg).max())
    # a last-layer RZ shift changes no probability: exactly 0
    rz_last = Gd.view(B, L, n, 2)[:, L - 1, :, 1]
    # the autograd path against the adjoint of the exact simulators: both lie within atol * sum|gE| of the truth
    grads = []
    for kw in ({}, {"diff_method": "parameter_shift"}):
        xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
        (qsim(xa, wa, "hip", **kw) * gE.to(cuda)).sum().backward()
        grads.append((xa.grad.cpu().double(), wa.grad.cpu().double()))
    edx = float(((grads[0][0] - grads[1][0]).abs() / sg).max())
    edw = float((grads[0][1] - grads[1][1]).abs().max() / sg.sum())
    print(f"n={n} L={L} B={B} G={G}: |dp|={ep:.2e} |dE|={eE:.2e} |dG|/sum|gE|={eG:.2e} "
          f"|dx - adjoint|/sum|gE|={edx:.2e} |dw - adjoint|/sum|gE|={edw:.2e}")
    assert ep <= atol and eE <= atol and eG <= atol
    assert torch.equal(rz_last, torch.zeros_like(rz_last))
    assert torch.equal(grads[1][0].float(), Gd[:, 0:2 * n:2].cpu())
    assert edx <= 2 * atol and edw <= 2 * atol
    if G:
        assert float(grads[1][1][1:].abs().max()) == 0   # the master gradient sits in group 0


@pytest.mark.parametrize("shots", [65, 1025])
@pytest.mark.parametrize("n,L,B,G", CASES)
def test_finite_shots(cuda, n, L, B, G, shots):
    x, w, gE, _, _, G_exact, sigma1 = case(n, L, B, G)
    P = 2 * n * L
    Gd, Epm, probs = launch(x.to(cuda), w.to(cuda), gE.to(cuda), shots, SEED_HI, CTR_HI)
    # the stream contract, against the existing sampler, with no tolerance
    for p in range(P):
        for s in range(2):
            ref = sample_z(probs[:, p, s].contiguous(), shots, SEED_HI, pshift_counter(CTR_HI, p, s))
            assert torch.equal(Epm[:, p, s], ref), (p, s)
    Epm, Gd = Epm.cpu().double(), Gd.cpu().double()
    k = Epm * shots
    assert float((k - k.round()).abs().max()) <= 1e-3 and bool(((k.round().long() - shots) % 2 == 0).all())
    sg = gE.double().abs().sum(1, keepdim=True)
    contr = (0.5 * (Epm[:, :, 0] - Epm[:, :, 1]) * gE.double()[:, None, :]).sum(-1)
    eG = float(((Gd - contr).abs() / sg).max())
    ratio = float(((Gd - G_exact).abs() / (6 * sigma1 / math.sqrt(shots) + 4 * sg / shots)).max())
    print(f"n={n} L={L} B={B} G={G} shots={shots}: |G - Epm.gE|/sum|gE|={eG:.2e} (bound {n * 2.0 ** -23:.2e}); "
          f"max |G - G_exact| / bound = {ratio:.3f}")
    assert eG <= n * 2.0 ** -23   # fp32 summation error only
    assert ratio <= 1.0
    # a row's shots do not depend on B
    G1, _, _ = launch(x[:1].to(cuda), (w if G == 0 else w[0]).to(cuda), gE[:1].to(cuda), shots, SEED_HI, CTR_HI,
                      want=(False, False))
    assert torch.equal(G1.cpu().double(), Gd[:1])


@pytest.mark.parametrize("shots", [0, 65])
@pytest.mark.parametrize("n,L,B,G", [(5, 3, 3, 0), (12, 2, 2, 0), (8, 3, 6, 3)])
def test_mask_and_need_dx(cuda, n, L, B, G, shots):
    x, w, gE = (t.to(cuda) for t in case(n, L, B, G)[:3])
    full = launch(x, w, gE, shots, SEED_HI, CTR_HI)
    mask = torch.rand(L, n, 2, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[0] = False           # all of layer 0
    mask[L - 1, 0] = True     # (with L = 1 layer 0 keeps one qubit)
    m8 = mask.reshape(-1).to(device=cuda, dtype=torch.uint8)
    ry0 = torch.zeros(L, n, 2, dtype=torch.bool)
    ry0[0, :, 0] = True
    for need_dx in (True, False):
        ran = (mask | ry0 if need_dx else mask).reshape(-1).to(cuda)
        assert bool(ran.any()) and not bool(ran.all())
        Gm, Em, pm = launch(x, w, gE, shots, SEED_HI, CTR_HI, mask=m8, need_dx=need_dx, fill=SENTINEL)
        assert torch.equal(Gm[:, ran], full[0][:, ran]) and torch.equal(Gm[:, ~ran], torch.zeros_like(Gm[:, ~ran]))
        assert torch.equal(Em[:, ran], full[1][:, ran]) and torch.equal(pm[:, ran], full[2][:, ran])
        assert bool((Em[:, ~ran] == SENTINEL).all()) and bool((pm[:, ~ran] == SENTINEL).all())
    # the autograd path: masked entries exactly 0, the others and dx unchanged
    kw = dict(diff_method="parameter_shift", shots=shots or None, seed=SEED_HI, counter=CTR_HI)
    out = []
    for sm in (None, mask):
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        (qsim(xa, wa, "hip", shift_mask=sm, **kw) * gE).sum().backward()
        out.append((xa.grad, wa.grad if G == 0 else wa.grad[0]))
    mk = mask.to(cuda)
    assert torch.equal(out[1][0], out[0][0])
    assert torch.equal(out[1][1][mk], out[0][1][mk]) and float(out[1][1][~mk].abs().max()) == 0


@pytest.mark.parametrize("B", [1366, 2048, 4096])
def test_workgroup_split_is_invisible(cuda, B):
    """The launcher splits a layer's qubits over 3, 2 and 1 workgroups at these batch sizes (3 at the small ones
    above): the rows they share with a small batch are the same to the bit."""
    n, L = 3, 2
    g = torch.Generator().manual_seed(5)
    x, gE = torch.rand(B, n, generator=g) * 2 - 1, torch.rand(B, n, generator=g) * 2 - 1
    x, gE, w = x.to(cuda), gE.to(cuda), (torch.rand(L, n, 2, generator=g) * 2 * math.pi).to(cuda)
    for shots in (0, 65):
        big = launch(x, w, gE, shots, SEED_HI, CTR_HI)
        small = launch(x[:3].contiguous(), w, gE[:3].contiguous(), shots, SEED_HI, CTR_HI)
        for a, b in zip(big, small):
            assert torch.equal(a[:3], b)
    tail = launch(x[-1:].contiguous(), w, gE[-1:].contiguous())
    for a, b in zip(big if shots == 0 else launch(x, w, gE), tail):
        assert torch.equal(a[-1:], b)


def test_graph_capture_with_device_counter(cuda):
    n, L, B = 8, 3, 4
    x, w, gE = (t.to(cuda) for t in case(n, L, B, 0)[:3])
    shots = 257
    eager = [launch(x, w, gE, shots, SEED_HI, k, want=(False, False))[0] for k in range(3)]
    ctr = torch.zeros((), dtype=torch.int64, device=cuda)
    G = torch.empty(B, 2 * n * L, device=cuda)
    Q.hip_qsim_pshift(x, w, gE, G, shots=shots, seed=SEED_HI, counter_ptr=nat.ptr(ctr))   # (first launch outside)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Q.hip_qsim_pshift(x, w, gE, G, shots=shots, seed=SEED_HI, counter_ptr=nat.ptr(ctr))
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
    x, w, gE = (t.to(cuda) for t in case(n, L, B, 0)[:3])
    clean = [launch(x, w, gE, shots, SEED_HI, CTR_HI) for shots in (0, 257)]
    try:
        nat.set_lds_poison(pattern)
        poisoned = [launch(x, w, gE, shots, SEED_HI, CTR_HI) for shots in (0, 257)]
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    for c, p in zip(clean, poisoned):
        for a, b in zip(c, p):
            assert torch.equal(a, b)


def test_module_backward_is_the_kernel(cuda):
    torch.manual_seed(0)
    n, L, B, shots = 8, 3, 6, 256
    m = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False, shots=shots,
                 diff_method="parameter_shift").to(cuda).train()
    m.qlayer.manual_shot_seed(SEED_HI)
    seen = {}

    def hook(_, inp, out):
        seen["angles"] = inp[0].detach().float().contiguous()
        out.register_hook(lambda g: seen.__setitem__("gE", g.detach().float().contiguous()))

    m.qlayer.register_forward_hook(hook)
    inp = torch.randn(B, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    torch.nn.functional.nll_loss(m(inp), torch.arange(B, device=cuda) % 3).backward()
    G, _, _ = launch(seen["angles"], m.qlayer.weights.detach().contiguous(), seen["gE"], shots, SEED_HI, 0,
                     want=(False, False))
    G = G.double()
    err = (m.qlayer.weights.grad.reshape(-1).double() - G.sum(0)).abs()
    assert bool((err <= B * 2.0 ** -23 * G.abs().sum(0)).all())   # fp32 summation over the batch
    assert float(G.abs().max()) > 0 and m.preprocess[0].weight.grad is not None
    assert bool(torch.isfinite(m.preprocess[0].weight.grad).all())


def test_range_checks(cuda):
    x, w = torch.zeros(2, 13, device=cuda), torch.zeros(1, 13, 2, device=cuda)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", diff_method="parameter_shift")
    # the entry point itself refuses what is out of range (hipErrorInvalidValue = 1), launching nothing
    x, w, gE = torch.zeros(1, 2, device=cuda), torch.zeros(8192, 2, 2, device=cuda), torch.zeros(1, 2, device=cuda)
    G = torch.empty(1, 4 * 8192, device=cuda)
    with pytest.raises(RuntimeError, match="status 1"):
        Q.hip_qsim_pshift(x, w, gE, G)                       # 2P + 1 = 2^16 + 1 stream ids
    with pytest.raises(RuntimeError, match="status 1"):
        Q.hip_qsim_pshift(x, w[:2], gE, G, shots=(1 << 20) + 1)
