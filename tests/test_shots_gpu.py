"""Finite-shot measurement on the HIP kernels (csrc/hip/qsim_shots.hip): probabilities against the fp64 oracle, the
sampler against the C++ implementation of the same integer contract (bit for bit), the fused kernel against the
two-stage pair, graph capture with a device counter, straight-through gradients, LDS poisoning and inference."""
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                             QSC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (counter_add, qsim, qsim_probs,
                                                                                         sample_z, z_signs)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference

pytestmark = pytest.mark.gpu

SEED = 1234
SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32
# (n, L, B, G): G > 0 = grouped weights (G, L, n, 2)
PROB_CASES = [(2, 1, 3, 0), (5, 3, 5, 0), (6, 3, 4, 0), (8, 3, 16, 0), (10, 2, 4, 0), (11, 2, 3, 0), (12, 3, 3, 0),
              (8, 3, 6, 3)]


def inputs(n, L, B, G=0):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if G == 0 else torch.rand(G, L, n, 2) * 2 * math.pi
    return x, w


def shot_bound(E_exact, shots):
    return 6 * torch.sqrt((1 - E_exact.double() ** 2).clamp_min(0) / shots) + 4 / shots


def fused(x, w, shots, seed, ctr0):
    """(E, counts) of the fused kernel (raw launcher: the autograd wrapper does not return counts)."""
    B, n = x.shape
    E = torch.empty(B, n, device=x.device)
    c = torch.empty(B, n, device=x.device, dtype=torch.int32)
    Q.hip_qsim_shots_fwd(x.contiguous(), w.contiguous(), E, c, shots, seed, ctr0, None, Q.wgroup_of(x, w))
    return E, c


@pytest.mark.parametrize("n,L,B,G", PROB_CASES)
def test_probs_match_fp64_oracle(cuda, n, L, B, G):
    x, w = inputs(n, L, B, G)
    atol = 2e-5 if n <= 10 else 5e-5
    p_cpu = qsim_probs(x, w, "cpu")
    E_cpu = qsim(x, w, "cpu")
    p = qsim_probs(x.to(cuda), w.to(cuda), "hip")
    assert p.dtype == torch.float32 and p.shape == (B, 1 << n)
    p = p.cpu().double()
    err = float((p - p_cpu).abs().max())
    errE = float((p @ z_signs(n, dtype=torch.float64) - E_cpu.double()).abs().max())
    errS = float((p.sum(1) - 1).abs().max())
    print(f"n={n} L={L} B={B} G={G}: |dp|={err:.2e} |dE|={errE:.2e} |sum-1|={errS:.2e}")
    assert err <= atol and errE <= atol and errS <= 1e-5


@pytest.mark.parametrize("n", [2, 5, 6, 8, 12])
def test_sampler_matches_cpu_bit_for_bit(cuda, n):
    for B in (1, 3):
        x, w = inputs(n, 3, B)
        p = qsim_probs(x.to(cuda), w.to(cuda), "hip")
        p_host = p.cpu()
        for shots in (1, 63, 64, 65, 257, 4096):
            E, c = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
            Er, cr = sample_z(p_host, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
            assert torch.equal(c.cpu(), cr), (n, B, shots)
            assert torch.equal(E.cpu(), Er), (n, B, shots)


@pytest.mark.parametrize("n,L,B,G", PROB_CASES)
def test_fused_equals_two_stage(cuda, n, L, B, G):
    x, w = inputs(n, L, B, G)
    x, w = x.to(cuda), w.to(cuda)
    p = qsim_probs(x, w, "hip")
    for shots in (65, 4096):
        E2, c2 = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
        E1, c1 = fused(x, w, shots, SEED_HI, CTR_HI)
        assert torch.equal(c1, c2) and torch.equal(E1, E2), (n, shots)
        assert torch.equal(qsim(x, w, "hip", shots=shots, seed=SEED_HI, counter=CTR_HI), E1)


@pytest.mark.parametrize("n,L,B", [(8, 3, 16), (12, 3, 3)])
def test_statistical_bound_hip(cuda, n, L, B):
    shots = 4096
    x, w = inputs(n, L, B)
    E_exact = qsim(x, w, "cpu")
    E = qsim(x.to(cuda), w.to(cuda), "hip", shots=shots, seed=SEED, counter=0).cpu()
    ratio = (E.double() - E_exact.double()).abs() / shot_bound(E_exact, shots)
    print(f"n={n}: max |E_shots - E_exact| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


def test_graph_capture_with_device_counter(cuda):
    x, w = inputs(8, 3, 16)
    x, w = x.to(cuda), w.to(cuda)
    eager = [qsim(x, w, "hip", shots=257, seed=SEED, counter=k) for k in range(3)]
    ctr = torch.zeros((), dtype=torch.int64, device=cuda)
    qsim(x, w, "hip", shots=257, seed=SEED, counter=ctr)   # (first launch outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = qsim(x, w, "hip", shots=257, seed=SEED, counter=ctr)
        counter_add(ctr, 1)
    ctr.zero_()
    got = []
    for _ in range(3):
        g.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    assert int(ctr) == 3
    for k in range(3):
        assert torch.equal(got[k], eager[k]), k
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2]) and not torch.equal(got[0], got[2])


@pytest.mark.parametrize("n,L,B", [(8, 3, 16), (12, 3, 3)])
def test_gradients_are_exact_hip(cuda, n, L, B):
    x, w = inputs(n, L, B)
    g = torch.rand(B, n, generator=torch.Generator().manual_seed(2)).to(cuda)
    grads = []
    for shots in (None, 4096):
        xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
        (qsim(xa, wa, "hip", shots=shots, seed=SEED) * g).sum().backward()
        grads.append((xa.grad, wa.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_range_checks(cuda):
    x, w = inputs(13, 1, 2)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x.to(cuda), w.to(cuda), "hip", shots=16)
    with pytest.raises(NotImplementedError, match="12"):
        qsim_probs(x.to(cuda), w.to(cuda), "hip")
    # the entry points themselves refuse what is out of range (hipErrorInvalidValue = 1), launching nothing
    x, w = inputs(4, 2, 2)
    x, w = x.to(cuda), w.to(cuda)
    E = torch.empty(2, 4, device=cuda)
    for shots in (0, (1 << 20) + 1):
        with pytest.raises(RuntimeError, match="status 1"):
            Q.hip_qsim_shots_fwd(x, w, E, None, shots)
        with pytest.raises(RuntimeError, match="status 1"):
            Q.hip_sample_z(torch.full((2, 16), 1 / 16, device=cuda), E, None, 4, shots)


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32, the largest CDF word)
@pytest.mark.parametrize("n,L,B", [(5, 3, 5), (8, 3, 16), (12, 3, 3)])
def test_lds_poison(cuda, n, L, B, pattern):
    x, w = inputs(n, L, B)
    x, w = x.to(cuda), w.to(cuda)
    _, clean = fused(x, w, 257, SEED, 0)
    p_clean = qsim_probs(x, w, "hip")
    try:
        nat.set_lds_poison(pattern)
        _, poisoned = fused(x, w, 257, SEED, 0)
        p_poisoned = qsim_probs(x, w, "hip")
        _, two_stage = sample_z(p_poisoned, 257, seed=SEED, return_counts=True)
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    assert torch.equal(poisoned, clean)
    assert torch.equal(p_poisoned, p_clean)
    assert torch.equal(two_stage, clean)


# ------------------------------------------------------------------------------- inference
N_INFER, CHUNK = 700, 576


@pytest.fixture(scope="module")
def engine(cuda):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(cuda).eval() for _ in range(3)]
    fc = FC_P128(128).to(cuda).eval()
    qsc = QSC_P128(8, 3, 3, False, False, 128).to(cuda).eval()
    eng = HIPInference(convs, fc, 128, cuda, chunk=CHUNK, qsc=qsc)
    x = torch.randn(N_INFER, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    return eng, qsc, x


def _host_recompute(eng, qsc, x, shots, seed):
    """Engine angles -> qsim(cpu, shots, counter = chunk index) -> head -> (argmax, top-two log-probability gap)."""
    preds, gaps = [], []
    w = qsc.qlayer.weights.detach().cpu()
    for c, lo in enumerate(range(0, x.shape[0], CHUNK)):
        n = min(CHUNK, x.shape[0] - lo)
        eng._load(x, lo, n)
        eng.qsc.infer(eng.xq, eng.pred)
        ang = eng.qsc.angles.detach().cpu()
        E = qsim(ang, w, "cpu", shots=shots, seed=seed, counter=c)
        logp = torch.log_softmax(E.double() @ qsc.classifier.weight.detach().cpu().double().T
                                 + qsc.classifier.bias.detach().cpu().double(), dim=1)[:n]
        top = logp.topk(2, dim=1).values
        preds.append(logp.argmax(1))
        gaps.append(top[:, 0] - top[:, 1])
    return torch.cat(preds), torch.cat(gaps)


@pytest.mark.parametrize("shots", [64, 1024])
def test_inference_with_shots(engine, shots):
    eng, qsc, x = engine
    with torch.no_grad():
        a = eng.classify(x, "quantum", shots=shots, seed=SEED)
        b = eng.classify(x, "quantum", shots=shots, seed=SEED)
        other = eng.classify(x, "quantum", shots=shots, seed=SEED + 1)
        exact = eng.classify(x, "quantum")
        ref, gap = _host_recompute(eng, qsc, x, shots, SEED)
        agree = {s: float((eng.classify(x, "quantum", shots=s, seed=SEED) == exact).float().mean())
                 for s in (1, 1 << 20)}
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    keep = gap >= 1e-3
    excluded = 1 - float(keep.float().mean())
    msg = (f"shots={shots}: excluded {excluded:.4f}; agreement with the exact classify: shots=1 {agree[1]:.4f}, "
           f"shots={shots} {float((a == exact).float().mean()):.4f}, shots=2^20 {agree[1 << 20]:.4f}; "
           f"differs from seed+1 on {float((a != other).float().mean()):.4f}")
    print(msg)
    assert excluded <= 0.02, msg
    assert torch.equal(a.cpu()[keep], ref[keep]), msg


def test_shots_are_for_the_quantum_classifier(engine):
    eng, _, x = engine
    with pytest.raises(ValueError):
        eng.classify(x, "classical", shots=16)
