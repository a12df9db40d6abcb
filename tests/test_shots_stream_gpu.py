"""Finite-shot measurement at n = 13..16 on the streamed simulator (csrc/hip/qsim_stream.hip's probabilities pass,
csrc/hip/qsim_stream_shots.hip's block sampler): probabilities against the fp64 oracle, the sampler against the host
sampler bit for bit, fused == two-stage, the statistical bound, straight-through gradients, graph capture, LDS
poisoning, the entry points' range checks, the refusals that remain, and inference through the fused QSC step."""
import ctypes
import itertools

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, counter_add, qsim,
                                                                                         qsim_probs, sample_z, z_signs)

from test_shots_gpu import CTR_HI, SEED, SEED_HI, fused, inputs, shot_bound
from test_shots_stream_cpu import check_degenerate, degenerate_rows

pytestmark = pytest.mark.gpu

# (n, L, B, G): n = 13 two tiles (one block pair), 16 sixteen; L = 2 the generating pass A feeds the probabilities
# pass, L = 3 adds a loaded pass A and an intermediate pass B; G > 0 = grouped weights (G, L, n, 2)
SHAPES = [(n, L, B, 0) for n, L, B in itertools.product((13, 14, 16), (2, 3), (1, 3))] + [(16, 3, 4, 2)]
_p, _i, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64


@pytest.fixture(scope="module")
def oracle():
    """(x, w, p_cpu fp64, E_cpu) per shape, computed once and left unchanged."""
    memo = {}

    def get(n, L, B, G):
        if (n, L, B, G) not in memo:
            x, w = inputs(n, L, B, G)
            memo[(n, L, B, G)] = (x, w, qsim_probs(x, w, "cpu"), qsim(x, w, "cpu"))
        return memo[(n, L, B, G)]
    return get


@pytest.mark.parametrize("n,L,B,G", SHAPES)
def test_probs_match_fp64_oracle(cuda, oracle, n, L, B, G):
    """|p z - E_cpu| <= 5e-5 and |sum p - 1| <= 1e-5 (the project's tolerances for the streamed simulator), and the
    L1 distance sum_k |p_k - p_cpu,k| <= n L 2^-17: with G = 2 n L rotations the fp32 state carries
    |d psi| <= G eps, so sum | |psi~_k|^2 - |psi_k|^2 | <= |d psi| (2 + |d psi|) ~ 2 G eps, at eps = 2^-19 per
    rotation (__sincosf's absolute error, about 2^-21.4 per entry, plus fp32 complex arithmetic, with headroom)."""
    x, w, p_cpu, E_cpu = oracle(n, L, B, G)
    p = qsim_probs(x.to(cuda), w.to(cuda), "hip")
    assert p.dtype == torch.float32 and p.shape == (B, 1 << n)
    p = p.cpu().double()
    errE = float((p @ z_signs(n, dtype=torch.float64) - E_cpu.double()).abs().max())
    errS = float((p.sum(1) - 1).abs().max())
    errL1 = float((p - p_cpu).abs().sum(1).max())
    bound = n * L * 2.0 ** -17
    print(f"n={n} L={L} B={B} G={G}: |dE|={errE:.2e} |sum-1|={errS:.2e} L1={errL1:.2e} (bound {bound:.2e}, "
          f"ratio {errL1 / bound:.3f})")
    assert errE <= 5e-5 and errS <= 1e-5 and errL1 <= bound


@pytest.mark.parametrize("n", [13, 14, 16])
def test_sampler_matches_cpu_bit_for_bit(cuda, n):
    for B in (1, 3):
        x, w = inputs(n, 2, B)
        p = qsim_probs(x.to(cuda), w.to(cuda), "hip")
        p_host = p.cpu()
        for shots in (1, 63, 64, 65, 257, 4096):
            E, c = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
            Er, cr = sample_z(p_host, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
            assert torch.equal(c.cpu(), cr), (n, B, shots)
            assert torch.equal(E.cpu(), Er), (n, B, shots)


@pytest.mark.parametrize("n", [13, 16])
@pytest.mark.parametrize("shots", [1, 63, 257])
def test_degenerate_distributions_gpu(cuda, n, shots):
    p = degenerate_rows(n)
    E, c = sample_z(p.to(cuda), shots, seed=SEED, return_counts=True)
    Er, cr = sample_z(p, shots, seed=SEED, return_counts=True)
    assert torch.equal(c.cpu(), cr) and torch.equal(E.cpu(), Er)
    check_degenerate(n, shots, E.cpu(), c.cpu())


@pytest.mark.parametrize("n,L,B,G", SHAPES)
def test_fused_equals_two_stage(cuda, n, L, B, G):
    x, w = inputs(n, L, B, G)
    x, w = x.to(cuda), w.to(cuda)
    p = qsim_probs(x, w, "hip")
    for shots in (65, 4096):
        E2, c2 = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
        E1, c1 = fused(x, w, shots, SEED_HI, CTR_HI)
        assert torch.equal(c1, c2) and torch.equal(E1, E2), (n, shots)
        assert torch.equal(qsim(x, w, "hip", shots=shots, seed=SEED_HI, counter=CTR_HI), E1)


@pytest.mark.parametrize("n,L,B", [(13, 2, 3), (16, 3, 3)])   # (tests/test_shots_stream_cpu.py: the host twins)
def test_statistical_bound_hip(cuda, n, L, B):
    shots = 4096
    x, w = inputs(n, L, B)
    E_exact = qsim(x, w, "cpu")
    E = qsim(x.to(cuda), w.to(cuda), "hip", shots=shots, seed=SEED, counter=0).cpu()
    ratio = (E.double() - E_exact.double()).abs() / shot_bound(E_exact, shots)
    print(f"n={n}: max |E_shots - E_exact| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("n,L,B", [(13, 2, 2), (16, 3, 2)])
def test_gradients_are_exact_hip(cuda, n, L, B):
    x, w = inputs(n, L, B)
    g = torch.rand(B, n, generator=torch.Generator().manual_seed(2)).to(cuda)
    grads = []
    for shots in (None, 4096):
        xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
        (qsim(xa, wa, "hip", shots=shots, seed=SEED) * g).sum().backward()
        grads.append((xa.grad, wa.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_graph_capture_with_device_counter(cuda):
    x, w = inputs(13, 2, 2)
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


@pytest.mark.parametrize("pattern", [True, 0xFFFFFFFF])   # (0xFFFFFFFF: NaN as fp32, the largest CDF word)
@pytest.mark.parametrize("n,L,B", [(13, 2, 2), (16, 3, 1)])
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


def test_entry_points_refuse_out_of_range(cuda):
    """Each raw entry point returns hipErrorInvalidValue (1) and writes nothing for n = 12 / 17, L = 1, 2 n L > 1024,
    shots 0 / 2^20 + 1, B = 0, a null workspace and a wgroup that does not divide B."""
    lib = nat.hip_lib()
    f_probs = nat.fn(lib, "qd_qsim_stream_probs", [_p, _p, _p, _i, _i, _i, _i, _p, _p])
    f_samp = nat.fn(lib, "qd_stream_sample_z", [_p, _p, _p, _i, _i, _i, _u64, _u64, _p, _p, _p])
    f_fused = nat.fn(lib, "qd_qsim_stream_shots_fwd", [_p, _p, _p, _p, _i, _i, _i, _i, _i, _u64, _u64, _p, _p, _p])
    B = 3
    x = torch.zeros(B, 17, device=cuda)
    w = torch.zeros(33 * 16 * 2, device=cuda)
    bufs = {"probs": torch.full((B << 13,), 7.0, device=cuda), "E": torch.full((B, 17), 7.0, device=cuda),
            "counts": torch.full((B, 17), 7, device=cuda, dtype=torch.int32),
            "ws": torch.full((1 << 16,), 7, device=cuda, dtype=torch.uint8)}
    ref = {k: v.clone() for k, v in bufs.items()}
    ptr = {k: nat.ptr(v) for k, v in bufs.items()}
    st = nat.stream_ptr(cuda)
    # (n, L, shots, B, ws, wgroup)
    ok = (13, 2, 8, B, ptr["ws"], 0)
    bad = {"n=12": (12, 2, 8, B, ptr["ws"], 0), "n=17": (17, 2, 8, B, ptr["ws"], 0), "L=1": (13, 1, 8, B, ptr["ws"], 0),
           "2nL>1024": (16, 33, 8, B, ptr["ws"], 0), "shots=0": (13, 2, 0, B, ptr["ws"], 0),
           "shots>2^20": (13, 2, (1 << 20) + 1, B, ptr["ws"], 0), "B=0": (13, 2, 8, 0, ptr["ws"], 0),
           "ws=null": (13, 2, 8, B, None, 0), "wgroup": (13, 2, 8, B, ptr["ws"], 2)}
    assert ok not in bad.values()
    for name, (n, L, shots, b, ws, wg) in bad.items():
        if name not in ("shots=0", "shots>2^20"):
            assert f_probs(nat.ptr(x), nat.ptr(w), ptr["probs"], b, n, L, wg, ws, st) == 1, name
        if name not in ("L=1", "2nL>1024", "wgroup"):   # (the sampler has neither layers nor weights)
            assert f_samp(ptr["probs"], ptr["E"], ptr["counts"], b, n, shots, 1, 0, None, ws, st) == 1, name
        assert f_fused(nat.ptr(x), nat.ptr(w), ptr["E"], ptr["counts"], b, n, L, wg, shots, 1, 0, None, ws, st) == 1, name
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], ref[k]), k
    # the n <= 12 entry points keep refusing what lies above them
    f12 = nat.fn(lib, "qd_qsim_shots_fwd", [_p, _p, _p, _p, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    assert f12(nat.ptr(x), nat.ptr(w), ptr["E"], ptr["counts"], B, 13, 2, 0, 8, 1, 0, None, st) == 1


def test_refusals_that_remain(cuda):
    x, w = inputs(13, 1, 2)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x.to(cuda), w.to(cuda), "hip", shots=16)
    with pytest.raises(NotImplementedError, match="12"):
        qsim_probs(x.to(cuda), w.to(cuda), "hip")
    x, w = inputs(13, 2, 2)
    x, w = x.to(cuda), w.to(cuda)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=16, noise=NoiseModel(0.05, 0.1, 0.03, 0.05))
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=16, diff_method="parameter_shift")
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=16, diff_method="on_chip")
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x, w, "hip", shots=16, diff_method="noisy_adjoint", noise=NoiseModel(0.05, 0.1, 0.03, 0.05))


def test_inference_with_shots_16_qubits(cuda):
    """QSCStepHIP.infer(shots=) on a 16-qubit QSC: the circuit's E is the streamed fused forward's on the step's
    angles; the measured training step keeps its 12-qubit limit."""
    torch.manual_seed(0)
    B = 18
    m = QSC_P128(16, 2, 3, False, False, 128).to(cuda).eval()
    space = FlatParamSpace(list(m.named_parameters()), cuda)
    step = QSCStepHIP(m, space, B)
    x = torch.randn(B, 2, 16, 8, device=cuda)
    pred = torch.empty(B, dtype=torch.int64, device=cuda)
    step.infer(x, pred, shots=257, seed=SEED)
    E1, p1 = step.E.clone(), pred.clone()
    Er, _ = fused(step.angles, m.qlayer.weights.detach().contiguous(), 257, SEED, 0)
    assert torch.equal(E1, Er)
    assert float(E1.abs().max()) <= 1.0 and int(p1.min()) >= 0 and int(p1.max()) < 3
    step.infer(x, pred, shots=257, seed=SEED)
    assert torch.equal(step.E, E1) and torch.equal(pred, p1)
    step.infer(x, pred, shots=257, seed=SEED + 1)
    assert not torch.equal(step.E, E1)
    with pytest.raises(NotImplementedError, match="the HIP finite-shot kernels support n <= 12 qubits, got 16"):
        QSCStepHIP(m, space, B, shots=257)


def test_classify_with_shots_16_qubits(cuda):
    """HIPInference.classify(x, "quantum", shots=) on a 16-qubit QSC, two chunks (the last one partial): the argmax
    of the head over the streamed fused forward's E on the engine's angles, under the chunk index as the counter."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import Conv_P128, FC_P128
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference
    torch.manual_seed(0)
    chunk, N, shots = 18, 30, 257
    convs = [Conv_P128(128).to(cuda).eval() for _ in range(3)]
    qsc = QSC_P128(16, 2, 3, False, False, 128).to(cuda).eval()
    eng = HIPInference(convs, FC_P128(128).to(cuda).eval(), 128, cuda, chunk=chunk, qsc=qsc)
    x = torch.randn(N, 2, 16, 8, device=cuda, generator=torch.Generator(cuda).manual_seed(11))
    with torch.no_grad():
        a = eng.classify(x, "quantum", shots=shots, seed=SEED)
        b = eng.classify(x, "quantum", shots=shots, seed=SEED)
        w = qsc.qlayer.weights.detach().contiguous()
        cls = qsc.classifier
        for c, lo in enumerate(range(0, N, chunk)):
            n = min(chunk, N - lo)
            eng._load(x, lo, n)
            eng.qsc.infer(eng.xq, eng.pred)   # (the exact circuit: fills the angles)
            E, _ = fused(eng.qsc.angles, w, shots, SEED, c)
            logp = torch.log_softmax(E.double() @ cls.weight.double().T + cls.bias.double(), dim=1)[:n]
            top = logp.topk(2, dim=1).values
            keep = (top[:, 0] - top[:, 1]) >= 1e-3   # (a near tie may resolve differently in the fp32 head)
            assert torch.equal(a[lo:lo + n][keep], logp.argmax(1)[keep]), c
    assert a.shape == (N,) and torch.equal(a, b)
