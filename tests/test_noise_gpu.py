"""Gate and readout noise on the HIP kernel (csrc/hip/qsim_noise.hip): frames and probabilities against the C++
oracle of the same contract, sampling pinned bit for bit, zero thresholds against the noiseless shots kernel, graph
capture with a device counter, LDS poisoning, inference and range checks."""
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                             QSC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, counter_add,
                                                                                         noise_sites, pauli_frames,
                                                                                         qsim, qsim_probs,
                                                                                         sample_z_noisy)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference

pytestmark = pytest.mark.gpu

SEED = 1234
SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32
# (n, L, B, T, G): n = 5 has fewer amplitudes than threads, n = 9 is the first with more, n = 12 the LDS limit;
# L = 1 has only a last-layer frame (no trajectory rebuilds); G > 0 = grouped weights (G, L, n, 2)
CASES = [(2, 1, 3, 1, 0), (2, 2, 4, 3, 0), (5, 3, 6, 4, 0), (8, 3, 8, 16, 0), (9, 2, 4, 8, 0), (12, 2, 3, 4, 0),
         (8, 3, 6, 8, 3)]
GATES = dict(p1=0.2, p2=0.2)
NOISES = {"gates": NoiseModel(**GATES), "gates+readout": NoiseModel(readout01=0.1, readout10=0.3, **GATES)}


def inputs(n, L, B, G=0):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi if G == 0 else torch.rand(G, L, n, 2) * 2 * math.pi
    return x, w


def shots_of(T):
    return 257 if T == 1 else 32 * T


def noisy(x, w, noise, shots, T, seed=SEED_HI, ctr0=CTR_HI, cptr=None, debug=True):
    """(E, counts, probs_out, frames_out) of the raw launcher."""
    B, n = x.shape
    L = w.shape[-3]
    E = torch.empty(B, n, device=x.device)
    c = torch.empty(B, n, device=x.device, dtype=torch.int32)
    p = torch.full((B, T, 1 << n), float("nan"), device=x.device) if debug else None
    f = torch.full((B, T, L, 2), -1, device=x.device, dtype=torch.int32) if debug else None
    Q.hip_qsim_noisy_shots_fwd(x.contiguous(), w.contiguous(), E, c, noise, shots, T, seed, ctr0, cptr,
                               Q.wgroup_of(x, w), p, f)
    return E, c, p, f


_RUNS = {}


def run(cuda, case, which):
    """One launch per (case, noise model), shared by the tests below and left unchanged."""
    if (case, which) not in _RUNS:
        n, L, B, T, G = case
        x, w = inputs(n, L, B, G)
        out = noisy(x.to(cuda), w.to(cuda), NOISES[which], shots_of(T), T)
        torch.cuda.synchronize()
        _RUNS[(case, which)] = (x, w) + tuple(t.cpu() for t in out)
    return _RUNS[(case, which)]


@pytest.mark.parametrize("case", CASES)
def test_frames_equal_the_cpu_oracle(cuda, case):
    n, L, B, T, G = case
    _, _, _, _, _, frames = run(cuda, case, "gates")
    sites = noise_sites(NOISES["gates"], B, n, L, T, SEED_HI, CTR_HI)
    want = pauli_frames(sites)
    assert bool((sites != 0).any()) and bool((want != 0).any())
    assert torch.equal(frames, want)
    if L > 1:   # the shapes exercise both kinds of trajectory where they can
        rebuilt = (want[:, :, :L - 1] != 0).flatten(2).any(2)
        print(f"{case}: {int(rebuilt.sum())} of {rebuilt.numel()} trajectories rebuild the state")
        assert bool(rebuilt.any())


@pytest.mark.parametrize("case", CASES)
def test_probs_match_the_framed_fp64_oracle(cuda, case):
    n, L, B, T, G = case
    x, w, _, _, probs, frames = run(cuda, case, "gates")
    atol = 2e-5 if n <= 10 else 5e-5   # tests/test_shots_gpu.py test_probs_match_fp64_oracle's, for the same kernels
    want = qsim_probs(x.repeat_interleave(T, dim=0), w, "cpu", frames=frames.view(B * T, L, 2)).view(B, T, 1 << n)
    err = float((probs.double() - want).abs().max())
    errS = float((probs.double().sum(2) - 1).abs().max())
    print(f"{case}: |dp|={err:.2e} |sum-1|={errS:.2e}")
    assert err <= atol and errS <= 1e-5


@pytest.mark.parametrize("which", list(NOISES))
@pytest.mark.parametrize("case", CASES)
def test_sampling_is_pinned_bit_for_bit(cuda, case, which):
    n, L, B, T, G = case
    _, _, E, c, probs, frames = run(cuda, case, which)
    Er, cr = sample_z_noisy(probs, frames[:, :, L - 1, 0], NOISES[which], shots_of(T), SEED_HI, CTR_HI,
                            return_counts=True)
    assert torch.equal(c, cr), case
    assert torch.equal(E, Er), case
    if which == "gates+readout":   # the readout draws do change the counts
        assert not torch.equal(c, run(cuda, case, "gates")[3])
    else:                          # and the same frames were drawn: readout does not enter the gate streams
        assert torch.equal(frames, run(cuda, case, "gates+readout")[5])


@pytest.mark.parametrize("n,L,B,T", [(8, 3, 8, 16), (12, 3, 3, 8)])
def test_clean_and_rebuilt_trajectories_mix(cuda, n, L, B, T):
    """Realistic rates: some trajectories live on the noiseless CDF, the others rebuild the state."""
    noise = NoiseModel(p1=0.01, p2=0.02, readout01=0.02, readout10=0.02)
    shots = 32 * T
    x, w = inputs(n, L, B)
    E, c, probs, frames = (t.cpu() for t in noisy(x.to(cuda), w.to(cuda), noise, shots, T))
    want = pauli_frames(noise_sites(noise, B, n, L, T, SEED_HI, CTR_HI))
    rebuilt = (want[:, :, :L - 1] != 0).flatten(2).any(2)
    print(f"n={n}: {int(rebuilt.sum())} of {rebuilt.numel()} trajectories rebuild the state")
    assert bool(rebuilt.any()) and not bool(rebuilt.all())
    assert torch.equal(frames, want)
    pw = qsim_probs(x.repeat_interleave(T, dim=0), w, "cpu", frames=frames.view(B * T, L, 2)).view(B, T, 1 << n)
    assert float((probs.double() - pw).abs().max()) <= (2e-5 if n <= 10 else 5e-5)
    p0 = qsim_probs(x.to(cuda), w.to(cuda), "hip").cpu()   # the clean ones carry the noiseless kernel's values
    assert torch.equal(probs[~rebuilt], p0[:, None].expand(B, T, 1 << n)[~rebuilt])
    Er, cr = sample_z_noisy(probs, frames[:, :, L - 1, 0], noise, shots, SEED_HI, CTR_HI, return_counts=True)
    assert torch.equal(c, cr) and torch.equal(E, Er)


@pytest.mark.parametrize("n,L,B,T,p,oracle", [(2, 11, 2, 1024, 0.02, True), (12, 3, 1, 1024, 0.003, False)])
def test_frames_that_do_not_fit_the_lds_cache(cuda, n, L, B, T, p, oracle):
    """T (L - 1) frame words beyond the workgroup's LDS budget: the rebuilds draw their frames again."""
    noise = NoiseModel(p1=p, p2=p, readout01=0.02, readout10=0.02)
    shots = 4 * T
    x, w = inputs(n, L, B)
    E, c, probs, frames = (t.cpu() for t in noisy(x.to(cuda), w.to(cuda), noise, shots, T))
    want = pauli_frames(noise_sites(noise, B, n, L, T, SEED_HI, CTR_HI))
    rebuilt = (want[:, :, :L - 1] != 0).flatten(2).any(2)
    print(f"n={n} L={L} T={T}: {int(rebuilt.sum())} of {rebuilt.numel()} trajectories rebuild the state")
    assert bool(rebuilt.any()) and not bool(rebuilt.all())
    assert torch.equal(frames, want)
    if oracle:
        pw = qsim_probs(x.repeat_interleave(T, dim=0), w, "cpu", frames=frames.view(B * T, L, 2)).view(B, T, 1 << n)
        # fp32 rounding and the fast sincos' absolute error enter once per layer, so the error grows linearly in L:
        # the 2e-5 that holds at L = 3, scaled to this L
        assert float((probs.double() - pw).abs().max()) <= 2e-5 * L / 3
    else:   # (the fp64 oracle of 1024 twelve-qubit states is slow: the clean ones against the noiseless kernel)
        p0 = qsim_probs(x.to(cuda), w.to(cuda), "hip").cpu()
        assert torch.equal(probs[~rebuilt], p0[:, None].expand(B, T, 1 << n)[~rebuilt])
        assert float((probs.double().sum(2) - 1).abs().max()) <= 1e-5
    Er, cr = sample_z_noisy(probs, frames[:, :, L - 1, 0], noise, shots, SEED_HI, CTR_HI, return_counts=True)
    assert torch.equal(c, cr) and torch.equal(E, Er)


@pytest.mark.parametrize("n,L,B,G", [(2, 2, 3, 0), (5, 3, 5, 0), (8, 3, 16, 0), (12, 3, 3, 0), (8, 3, 6, 3)])
def test_zero_thresholds_equal_the_shots_kernel(cuda, n, L, B, G):
    shots = 96
    x, w = inputs(n, L, B, G)
    x, w = x.to(cuda), w.to(cuda)
    E0 = torch.empty(B, n, device=cuda)
    c0 = torch.empty(B, n, device=cuda, dtype=torch.int32)
    Q.hip_qsim_shots_fwd(x, w, E0, c0, shots, SEED_HI, CTR_HI, None, Q.wgroup_of(x, w))
    for T in (1, 3, shots // 4):
        E, c, _, frames = noisy(x, w, NoiseModel(), shots, T)
        assert torch.equal(c, c0) and torch.equal(E, E0), (n, T)
        assert not bool(frames.any())
        assert torch.equal(qsim(x, w, "hip", shots=shots, seed=SEED_HI, counter=CTR_HI, noise=NoiseModel(),
                                trajectories=T), E0)
    E0 = qsim(x, w, "hip", shots=257, seed=SEED)   # (T = 1: any shot count)
    assert torch.equal(qsim(x, w, "hip", shots=257, seed=SEED, noise=NoiseModel()), E0)


@pytest.mark.parametrize("n", range(2, 13))
def test_zero_thresholds_every_qubit_count(cuda, n):
    """Every instantiation builds the noiseless state to the shots kernel's bits."""
    x, w = inputs(n, 2, 3)
    x, w = x.to(cuda), w.to(cuda)
    E0 = torch.empty(3, n, device=cuda)
    c0 = torch.empty(3, n, device=cuda, dtype=torch.int32)
    Q.hip_qsim_shots_fwd(x, w, E0, c0, 256, SEED, 0)
    E, c, probs, _ = noisy(x, w, NoiseModel(), 256, 4, SEED, 0)
    assert torch.equal(c, c0) and torch.equal(E, E0)
    assert torch.equal(probs, qsim_probs(x, w, "hip")[:, None].expand(3, 4, 1 << n))


@pytest.mark.parametrize("n,L,B,T,G", [(8, 3, 8, 16, 0), (12, 3, 3, 8, 0), (5, 2, 6, 64, 3)])
def test_the_split_is_invisible(cuda, n, L, B, T, G):
    """One workgroup per sample, or 2 / 4 / 8 chunks of trajectories per sample: the same integers."""
    noise = NoiseModel(p1=0.01, p2=0.02, readout01=0.02, readout10=0.02)
    x, w = inputs(n, L, B, G)
    x, w = x.to(cuda), w.to(cuda)
    assert Q.noise_split(T, n) in (1, 2, 4, 8) and Q.noise_split(1, 12) == 1 and Q.noise_split(3, 12) == 1
    assert Q.noise_split(16, 12) == 4 and Q.noise_split(64, 12) == 8 and Q.noise_split(64, 8) == 1
    outs, zero = {}, {}
    E0 = torch.empty(B, n, device=cuda)
    c0 = torch.empty(B, n, device=cuda, dtype=torch.int32)
    Q.hip_qsim_shots_fwd(x, w, E0, c0, 32 * T, SEED_HI, CTR_HI, None, Q.wgroup_of(x, w))
    try:
        for split in (0, 1, 2, 4, 8):
            Q.noise_force_split(split)
            outs[split] = noisy(x, w, noise, 32 * T, T)
            zero[split] = noisy(x, w, NoiseModel(), 32 * T, T)[:2]
            E_only = torch.empty(B, n, device=cuda)   # (counts are optional under every split)
            Q.hip_qsim_noisy_shots_fwd(x, w, E_only, None, noise, 32 * T, T, SEED_HI, CTR_HI, None, Q.wgroup_of(x, w))
            assert torch.equal(E_only, outs[split][0])
        Q.noise_force_split(8)
        with pytest.raises(RuntimeError, match="status 1"):   # 8 chunks do not divide 12 trajectories
            noisy(x, w, noise, 48, 12)
        with pytest.raises(RuntimeError, match="status 1"):
            Q.noise_force_split(3)
        torch.cuda.synchronize()
    finally:
        Q.noise_force_split(0)
    for split in (0, 2, 4, 8):
        for a, b in zip(outs[split], outs[1]):
            assert torch.equal(a, b), split
    for split in zero:
        assert torch.equal(zero[split][0], E0) and torch.equal(zero[split][1], c0), split


def test_debug_outputs_do_not_change_the_result(cuda):
    x, w = inputs(8, 3, 8)
    x, w = x.to(cuda), w.to(cuda)
    noise = NOISES["gates+readout"]
    E, c, _, _ = noisy(x, w, noise, 512, 16)
    E2, c2, _, _ = noisy(x, w, noise, 512, 16, debug=False)
    assert torch.equal(E, E2) and torch.equal(c, c2)
    assert torch.equal(qsim(x, w, "hip", shots=512, seed=SEED_HI, counter=CTR_HI, noise=noise, trajectories=16), E)


def test_graph_capture_with_device_counter(cuda):
    x, w = inputs(8, 3, 16)
    x, w = x.to(cuda), w.to(cuda)
    kw = dict(shots=256, seed=SEED, noise=NOISES["gates+readout"], trajectories=16)
    eager = [qsim(x, w, "hip", counter=k, **kw) for k in range(3)]
    ctr = torch.zeros((), dtype=torch.int64, device=cuda)
    qsim(x, w, "hip", counter=ctr, **kw)   # (first launch, and the thresholds' upload, outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = qsim(x, w, "hip", counter=ctr, **kw)
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
@pytest.mark.parametrize("n,L,B,T", [(8, 3, 8, 16), (12, 3, 3, 4)])
def test_lds_poison(cuda, n, L, B, T, pattern):
    x, w = inputs(n, L, B)
    x, w = x.to(cuda), w.to(cuda)
    noise = NOISES["gates+readout"]
    clean = noisy(x, w, noise, 32 * T, T)
    try:
        nat.set_lds_poison(pattern)
        poisoned = noisy(x, w, noise, 32 * T, T)
        torch.cuda.synchronize()
    finally:
        nat.set_lds_poison(None)
    for a, b in zip(poisoned, clean):
        assert torch.equal(a, b)


def test_gradients_are_the_noiseless_adjoint_hip(cuda):
    x, w = inputs(8, 3, 16)
    g = torch.rand(16, 8, generator=torch.Generator().manual_seed(2)).to(cuda)
    grads = []
    for kw in ({}, dict(shots=256, noise=NOISES["gates+readout"], trajectories=16)):
        xa, wa = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
        (qsim(xa, wa, "hip", seed=SEED, **kw) * g).sum().backward()
        grads.append((xa.grad, wa.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_range_checks(cuda):
    x, w = inputs(13, 1, 2)
    with pytest.raises(NotImplementedError, match="12"):
        qsim(x.to(cuda), w.to(cuda), "hip", shots=16, noise=NoiseModel(p1=0.01))
    # the entry point itself refuses what is out of range (hipErrorInvalidValue = 1), launching nothing
    x, w = inputs(4, 2, 2)
    x, w = x.to(cuda), w.to(cuda)
    E = torch.full((2, 4), 7.0, device=cuda)
    noise = NoiseModel(p1=0.01)
    for shots, T in ((64, 3), (64, 0), (4100, 1025), (30, 3), (0, 1), ((1 << 20) + 4, 1)):
        with pytest.raises(RuntimeError, match="status 1"):
            Q.hip_qsim_noisy_shots_fwd(x, w, E, None, noise, shots, T)
    torch.cuda.synchronize()
    assert bool((E == 7.0).all())


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


def test_inference_with_noise(engine):
    eng, qsc, x = engine
    noise = NoiseModel(p1=0.01, p2=0.05, readout01=0.02, readout10=0.03)
    kw = dict(shots=256, seed=SEED)
    with torch.no_grad():
        a = eng.classify(x, "quantum", noise=noise, trajectories=16, **kw)
        b = eng.classify(x, "quantum", noise=noise, trajectories=16, **kw)
        plain = eng.classify(x, "quantum", **kw)
        zero = eng.classify(x, "quantum", noise=NoiseModel(), trajectories=16, **kw)
        # the module path on the engine's angles: qsim under the chunk's counter, then the classifier head
        preds, gaps = [], []
        for c, lo in enumerate(range(0, x.shape[0], CHUNK)):
            n = min(CHUNK, x.shape[0] - lo)
            eng._load(x, lo, n)
            eng.qsc.infer(eng.xq, eng.pred)
            E = qsim(eng.qsc.angles.detach().clone(), qsc.qlayer.weights.detach(), "hip", counter=c, noise=noise,
                     trajectories=16, **kw)
            logp = torch.log_softmax(E.cpu().double() @ qsc.classifier.weight.detach().cpu().double().T
                                     + qsc.classifier.bias.detach().cpu().double(), dim=1)[:n]
            top = logp.topk(2, dim=1).values
            preds.append(logp.argmax(1))
            gaps.append(top[:, 0] - top[:, 1])
    torch.cuda.synchronize()
    ref, keep = torch.cat(preds), torch.cat(gaps) >= 1e-3
    excluded = 1 - float(keep.float().mean())
    print(f"excluded {excluded:.4f}; noisy differs from noiseless shots on {float((a != plain).float().mean()):.4f}")
    assert torch.equal(a, b)
    assert torch.equal(zero, plain)
    assert excluded <= 0.02
    assert torch.equal(a.cpu()[keep], ref[keep])
    with pytest.raises(ValueError):
        eng.classify(x, "quantum", noise=noise)   # noise needs shots
