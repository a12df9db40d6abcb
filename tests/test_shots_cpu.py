"""Finite-shot measurement of the QSC circuit on the host: the Philox generator, the sampling contract of
csrc/hip/qsim_shots.hip as implemented by the C++ oracle (csrc/cpu/qsim_cpu.cpp), the probability read-out,
straight-through gradients, and the module / config surface."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.config import EvalConfig
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128, QuantumLayer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (qsim, qsim_probs, sample_z,
                                                                                         z_signs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "quantum_distributed_machine_learning_ris_channel_estimation_amd", "csrc", "cpu")
SEED = 1234
STAT_CASES = [(2, 2, 3), (5, 3, 4), (6, 3, 4), (8, 3, 16), (10, 2, 4), (12, 3, 3)]


def inputs(n, L, B):
    torch.manual_seed(0)
    x = torch.rand(B, n) * 2 - 1
    w = torch.rand(L, n, 2) * 2 * math.pi
    return x, w


def shot_bound(E_exact, shots):
    """6 standard deviations of the shot mean of a +-1 variable with mean E_exact, plus 4 / shots."""
    return 6 * torch.sqrt((1 - E_exact.double() ** 2).clamp_min(0) / shots) + 4 / shots


def _philox(ctr, key):
    c = (ctypes.c_uint32 * 4)(*ctr)
    k = (ctypes.c_uint32 * 2)(*key)
    o = (ctypes.c_uint32 * 4)()
    nat.cpu_lib().qd_cpu_philox4x32(c, k, o)
    return list(o)


def test_philox_known_answers():
    assert _philox([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("n", [2, 6, 12])
@pytest.mark.parametrize("shots", [1, 63, 257])
def test_degenerate_distributions(n, shots):
    D = 1 << n
    hot = [0, D - 1, 5 % D]
    p = torch.zeros(4, D)
    for b, k in enumerate(hot):
        p[b, k] = 1.0
    p[3, 1::2] = torch.rand(D // 2, generator=torch.Generator().manual_seed(1)) + 0.1   # zero at every even index
    p[3] /= p[3].sum()
    E, c = sample_z(p, shots, seed=SEED, return_counts=True)
    assert torch.equal(E[0], torch.ones(n))
    assert torch.equal(E[1], -torch.ones(n))
    assert torch.equal(E[2], z_signs(n)[hot[2]])   # (index 5; at n = 2 its two low bits, index 1)
    assert float(E[3, 0]) == -1.0 and int(c[3, 0]) == shots


def test_determinism_and_counts():
    n, L, B, shots = 6, 3, 4, 4096
    x, w = inputs(n, L, B)
    p = qsim_probs(x, w, "cpu")
    E0, c0 = sample_z(p, shots, seed=SEED, counter=0, return_counts=True)
    E1, c1 = sample_z(p, shots, seed=SEED, counter=0, return_counts=True)
    E2, c2 = sample_z(p, shots, seed=SEED, counter=1, return_counts=True)
    assert torch.equal(c0, c1) and torch.equal(E0, E1)
    assert not torch.equal(c0, c2)
    assert not torch.equal(c0, sample_z(p, shots, seed=SEED + 1, counter=0, return_counts=True)[1])
    assert c0.dtype == torch.int32 and int(c0.min()) >= 0 and int(c0.max()) <= shots
    assert torch.equal(E0, (shots - 2 * c0).float() / float(shots))


@pytest.mark.parametrize("n,L,B", STAT_CASES)
def test_statistical_bound(n, L, B):
    shots = 4096
    x, w = inputs(n, L, B)
    E_exact = qsim(x, w, "cpu")
    E = qsim(x, w, "cpu", shots=shots, seed=SEED, counter=0)
    ratio = (E.double() - E_exact.double()).abs() / shot_bound(E_exact, shots)
    print(f"n={n} L={L} B={B}: max |E_shots - E_exact| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("n,L,B", STAT_CASES)
def test_probs_cpu(n, L, B):
    x, w = inputs(n, L, B)
    p = qsim_probs(x, w, "cpu")
    assert p.dtype == torch.float64 and p.shape == (B, 1 << n)
    assert float((p.sum(1) - 1).abs().max()) <= 1e-12
    assert float((p @ z_signs(n, dtype=torch.float64) - qsim(x, w, "cpu").double()).abs().max()) <= 1e-6


def test_probs_torch_backend():
    x, w = inputs(5, 3, 4)
    assert float((qsim_probs(x, w, "torch").double() - qsim_probs(x, w, "cpu")).abs().max()) < 1e-5


def test_gradients_are_exact():
    x, w = inputs(6, 3, 4)
    g = torch.rand(4, 6, generator=torch.Generator().manual_seed(2))
    grads = []
    for shots in (None, 4096):
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        (qsim(xa, wa, "cpu", shots=shots, seed=SEED) * g).sum().backward()
        grads.append((xa.grad, wa.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_grouped_weights_cpu():
    n, L, G, B = 4, 2, 3, 6
    x, w = inputs(n, L, B)
    wg = (w[None] + 0.1 * torch.arange(G)[:, None, None, None]).requires_grad_()
    E = qsim(x, wg, "cpu", shots=257, seed=SEED)
    p = torch.cat([qsim_probs(xc, wg[g].detach(), "cpu") for g, xc in enumerate(x.chunk(G))])
    assert torch.equal(E.detach(), sample_z(p, 257, seed=SEED))
    E.sum().backward()
    ge = wg.grad.clone()
    wg.grad = None
    qsim(x, wg, "cpu").sum().backward()
    assert torch.equal(ge, wg.grad)


def test_quantum_layer_shots():
    torch.manual_seed(0)
    exact = QuantumLayer(5, 2, backend="cpu")
    layer = QuantumLayer(5, 2, backend="cpu", shots=257)
    assert list(layer.state_dict().keys()) == list(exact.state_dict().keys())
    assert not list(layer.buffers()) and len(list(layer.parameters())) == 1
    assert "shots=257" in repr(layer) and "shot_seed=0" in repr(layer)
    x = torch.rand(3, 5) * 2 - 1
    layer.manual_shot_seed(7)
    a, b = layer(x), layer(x)
    assert not torch.equal(a, b)
    layer.manual_shot_seed(7)
    assert torch.equal(layer(x), a) and torch.equal(layer(x), b)
    assert "shot_seed=7" in repr(layer)
    layer.shots = None   # settable: back to the exact expectation
    assert torch.equal(layer(x), qsim(x, layer.weights, "cpu"))


def test_qsc_shots():
    torch.manual_seed(0)
    exact = QSC_P128(4, 2, 3, False, False, 128, backend="cpu").eval()
    model = QSC_P128(4, 2, 3, False, False, 128, backend="cpu", shots=63).eval()
    assert list(model.state_dict().keys()) == list(exact.state_dict().keys())
    assert model.qlayer.shots == 63
    x = torch.randn(5, 2, 16, 8)
    with torch.no_grad():
        model.qlayer.manual_shot_seed(3)
        a, b = model(x), model(x)
        assert not torch.equal(a, b)
        model.qlayer.manual_shot_seed(3)
        assert torch.equal(model(x), a)


def test_rejected_arguments():
    x, w = inputs(4, 2, 3)
    with pytest.raises(ValueError):
        qsim(x, w, "torch", shots=16)
    with pytest.raises(ValueError):
        qsim(x, w, "cpu", shots=(1 << 20) + 1)
    with pytest.raises(ValueError):
        sample_z(torch.full((1, 16), 1 / 16), 0)
    assert torch.equal(qsim(x, w, "cpu", shots=0), qsim(x, w, "cpu"))   # 0 / None: nothing changes


def test_eval_config_coerces_qsc_shots():
    cfg = EvalConfig().update_from_dict({"qsc_shots": "256"})
    assert cfg.qsc_shots == 256 and isinstance(cfg.qsc_shots, int)
    assert EvalConfig().qsc_shots == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_shots_driver_asan_ubsan(tmp_path):
    exe = tmp_path / "qsim_shots_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", os.path.join(CPU, "qsim_cpu.cpp"),
           os.path.join(CPU, "tests", "qsim_shots_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
