"""The exact density-matrix simulator on the host (ops/quantum.py ``qsim_mixed`` / ``qsim_mixed_probs`` / ``mixed_rows``
on ``cpu``: csrc/cpu/qsim_cpu.cpp qd_cpu_qsim_mixed_probs): the oracle against the dense NumPy references the sampling
tests already use, its exact properties, the module and config surface, the refusals, and the sanitizer driver."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.config import EvalConfig
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models import estimators
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                               QSC_P128, QuantumLayer,
                                                                                               SC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (MIXED_MAX_QUBITS, NoiseModel,
                                                                                         mixed_readout, mixed_rows,
                                                                                         qsim, qsim_mixed,
                                                                                         qsim_mixed_probs, z_signs)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.evaluate import model_val
from test_noise_cpu import _channel, circuit_ops, density_matrix_E, error_op, inputs
from test_onchip_cpu import density_matrix_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "quantum_distributed_machine_learning_ris_channel_estimation_amd", "csrc", "cpu")


def per_wire_noise(n):
    """Unequal per-wire rates with a 0 and a 0.5 in both gate rates."""
    return NoiseModel(p1=np.linspace(0.0, 0.5, n), p2=np.linspace(0.5, 0.0, n), readout01=np.linspace(0.0, 0.1, n),
                      readout10=np.linspace(0.5, 0.05, n))


def rates_of(noise, n):
    """The rates the kernels and the oracle use: the model's integer thresholds over 2^32 / 2^16 (exact in fp64)."""
    t1, t2, tro = noise.thresholds_host(n)
    return (t1.astype(np.float64) / 2.0 ** 32, t2.astype(np.float64) / 2.0 ** 32,
            tro[:, 0].astype(np.float64) / 65536.0, tro[:, 1].astype(np.float64) / 65536.0)


def expectation(x, w, noise):
    """E (B, n) fp64 of the oracle: its probabilities, the readout applied in fp64."""
    n = x.shape[1]
    c, d = mixed_readout(noise, n)
    return c * (qsim_mixed_probs(x, w, noise, "cpu") @ z_signs(n, dtype=torch.float64)) + d


def density_matrix_E_per_wire(x, w, n, L, p1, p2, r01, r10):
    """``density_matrix_E`` with a rate per wire, composed from its own pieces (tests/test_noise_cpu.py)."""
    D = 1 << n
    rho = np.zeros((D, D), dtype=complex)
    rho[0, 0] = 1
    for (l, q, k), M in circuit_ops(x, w, n, L):
        rho = M @ rho @ M.conj().T
        rho = _channel(rho, [error_op((l, q, k), c, n) for c in range(1, 16 if k else 4)], p2[q] if k else p1[q])
    bits = (np.arange(D)[:, None] >> np.arange(n)[None, :]) & 1
    return np.real(np.diag(rho)) @ np.where(bits == 1, -(1 - 2 * r10), 1 - 2 * r01)


# ------------------------------------------------------------------------------- against the dense references
@pytest.mark.parametrize("n,L", [(2, 1), (3, 2), (4, 2)])
def test_oracle_against_the_density_matrix(n, L):
    """Two fp64 evaluations of one definition: 1e-12."""
    B = 2
    x, w = inputs(n, L, B)
    xd, wd = x.double().numpy(), w.double().numpy()
    worst = 0.0
    # the sampling tests' own reference, one rate for all wires (and a readout rate per wire)
    for p1, p2 in ((0.05, 0.1), (0.5, 0.5), (0.0, 0.3), (0.25, 0.0)):
        noise = NoiseModel(p1, p2, readout01=np.linspace(0.0, 0.1, n), readout10=np.linspace(0.5, 0.05, n))
        q1, q2, r01, r10 = rates_of(noise, n)
        E = expectation(x, w, noise).numpy()
        for b in range(B):
            want = density_matrix_E(xd[b], wd, n, L, q1[0], q2[0], r01, r10)
            worst = max(worst, float(np.abs(E[b] - want).max()))
    # a rate per wire, 0 and 0.5 among them
    noise = per_wire_noise(n)
    E = expectation(x, w, noise).numpy()
    for b in range(B):
        want = density_matrix_E_per_wire(xd[b], wd, n, L, *rates_of(noise, n))
        worst = max(worst, float(np.abs(E[b] - want).max()))
        assert np.abs(want - qsim(x[b:b + 1], w, "cpu")[0].double().numpy()).max() > 0.01   # (the noise acts)
    print(f"n={n} L={L}: max |E - dm| = {worst:.2e}")
    assert worst <= 1e-12
    # the public function: the same numbers in fp32
    assert torch.equal(qsim_mixed(x, w, noise, "cpu"), torch.from_numpy(E).float())


def test_rows_against_the_density_matrix_gradient():
    """``mixed_rows`` on ``cpu`` against tests/test_onchip_cpu.py's dense derivative.  The rule is exact; what is left
    is the fp32 rounding of the shifted angle (|w +- pi/2| < 8: half an ulp is 2^-22, and |dE_j / dangle| <= 1, so
    each shifted E_j moves by at most 2^-22 and G by sum|gE| 2^-22) and of the fp32 result (2^-24 sum|gE|).  That is
    far inside the 6 sigma bound the sampled rows are held to there, which is asserted too."""
    n, L, B = 3, 2, 2
    x, w = inputs(n, L, B)
    gE = torch.rand(B, n, generator=torch.Generator().manual_seed(2)) * 2 - 1
    noise = NoiseModel(0.05, 0.1, 0.02, 0.03)
    p1, p2, r01, r10 = rates_of(noise, n)
    G = mixed_rows(x, w, gE, noise, "cpu")
    assert G.shape == (B, 2 * n * L) and G.dtype == torch.float32
    for b in range(B):
        want = density_matrix_gradient(x[b].double().numpy(), w.double().numpy(), gE[b].double().numpy(), n, L, p1[0],
                                       p2[0], r01[0], r10[0]).reshape(-1)
        ideal = density_matrix_gradient(x[b].double().numpy(), w.double().numpy(), gE[b].double().numpy(), n, L, 0, 0,
                                        0, 0).reshape(-1)
        sg = float(gE[b].double().abs().sum())
        err = float(np.abs(G[b].double().numpy() - want).max())
        bound = sg * (2.0 ** -22 + 2.0 ** -24)
        print(f"row {b}: max |G - dm| = {err:.3e}, bound {bound:.3e}; noiseless is {np.abs(ideal - want).max():.3e} away")
        assert err <= bound
        assert bound <= 6 * sg * math.sqrt((1 / 1024 + 1 / 16384) / (2 * 64))   # (the sampled rows' bound there)
        assert np.abs(ideal - want).max() > 1e3 * bound   # the noiseless gradient fails the check
    # autograd: dx the layer-0 RY columns, dw the rows' sum
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    (qsim_mixed(xa, wa, noise, "cpu") * gE).sum().backward()
    assert torch.equal(xa.grad, G[:, 0:2 * n:2]) and torch.equal(wa.grad, G.sum(0).view(L, n, 2))
    # grouped weights: every group's rows are those of its own call
    wg = torch.stack([w, w + 0.1])
    Gg = mixed_rows(x, wg, gE, noise, "cpu")
    assert torch.equal(Gg[0], G[0]) and torch.equal(Gg[1], mixed_rows(x[1:], w + 0.1, gE[1:], noise, "cpu")[0])


# ------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("n,L", [(2, 1), (5, 3), (8, 2)])
def test_zero_noise_is_the_exact_simulator(n, L):
    x, w = inputs(n, L, 3)
    E = qsim_mixed(x, w, NoiseModel(), "cpu")
    assert E.dtype == torch.float32 and E.shape == (3, n)
    assert float((E - qsim(x, w, "cpu")).abs().max()) <= 1e-6   # fp32 output of fp64 work


@pytest.mark.parametrize("n,L", [(2, 1), (4, 3), (7, 2)])
def test_probabilities(n, L):
    x, w = inputs(n, L, 3)
    for noise in (NoiseModel(), per_wire_noise(n), NoiseModel(0.5, 0.5)):
        p = qsim_mixed_probs(x, w, noise, "cpu")
        assert p.shape == (3, 1 << n) and p.dtype == torch.float64
        assert float((p.sum(1) - 1).abs().max()) <= 1e-12 and float(p.min()) >= -1e-15


def test_readout_alone_is_affine():
    n, L = 4, 2
    x, w = inputs(n, L, 3)
    ro = NoiseModel(readout01=[0.0, 0.1, 0.5, 0.02], readout10=[0.3, 0.0, 0.5, 0.05])
    c, d = mixed_readout(ro, n)
    assert torch.equal(qsim_mixed_probs(x, w, ro, "cpu"), qsim_mixed_probs(x, w, NoiseModel(), "cpu"))
    assert torch.equal(expectation(x, w, ro), c * expectation(x, w, NoiseModel()) + d)
    assert float(c[2]) == 0.0 and float(d[2]) == 0.0   # a wire read at random carries nothing


# ------------------------------------------------------------------------------- module and config
NOISE = NoiseModel(p1=0.02, p2=0.05, readout01=0.02, readout10=0.03)


def test_quantum_layer_exact_noise():
    torch.manual_seed(0)
    layer = QuantumLayer(4, 2, backend="cpu", noise=NOISE)
    assert layer.exact_noise is False
    x = torch.rand(3, 4) * 2 - 1
    with pytest.raises(ValueError, match="noise needs shots"):   # the default keeps the refusal
        layer(x)
    layer.exact_noise = True
    out = layer(x)
    assert torch.equal(out, qsim_mixed(x, layer.weights, NOISE, "cpu")) and out.requires_grad
    out.sum().backward()
    assert layer.weights.grad is not None and float(layer.weights.grad.abs().max()) > 0
    layer.shots = 64   # shots take over: the sampled path, untouched
    layer.manual_shot_seed(5)
    assert torch.equal(layer(x), qsim(x, layer.weights, "cpu", shots=64, seed=5, counter=0, noise=NOISE))
    layer.shots, layer.noise = None, None   # no noise: the exact noiseless circuit
    assert torch.equal(layer(x), qsim(x, layer.weights, "cpu"))
    assert not list(layer.buffers()) and len(list(layer.parameters())) == 1


def test_eval_config_and_model_val():
    assert EvalConfig().qsc_noise_exact is False
    for s, v in (("true", True), ("1", True), ("false", False), ("0", False)):
        cfg = EvalConfig().update_from_dict({"qsc_noise_exact": s})
        assert cfg.qsc_noise_exact is v
    with pytest.raises(ValueError):   # without the flag a rate without shots is still refused
        model_val(EvalConfig().update_from_dict({"qsc_noise_p1": 0.001}), device="cpu")
    with pytest.raises(ValueError, match="qsc_shots"):   # the exact channel takes no shots
        model_val(device="cpu", qsc_noise_exact=True, qsc_noise_p1=0.01, qsc_shots=64)
    mv = model_val(device="cpu", qsc_noise_exact="true", qsc_noise_p1="1e-2", qsc_noise_p2=0.05, qsc_readout01=0.02,
                   data_len_for_test=90)
    nm = mv.qsc_noise_model()
    assert isinstance(nm, NoiseModel) and nm.p1 == 1e-2 and nm.p2 == 0.05 and mv.qsc_noise_model() is nm
    assert model_val(device="cpu", qsc_noise_exact=True).qsc_noise_model() is None   # no rate: no noise


def test_evaluate_snr_with_the_exact_channel(monkeypatch):
    torch.manual_seed(0)
    convs = [Conv_P128(128).eval() for _ in range(3)]
    sc, fc = SC_P128(128).eval(), FC_P128(128).eval()
    qsc = QSC_P128(4, 2, 3, False, False, 128, backend="cpu").eval()
    calls = []
    real = estimators.qsim_mixed
    monkeypatch.setattr(estimators, "qsim_mixed", lambda x, w, noise, be=None: calls.append(noise) or real(x, w, noise, be))
    mv = model_val(device="cpu", qsc_noise_exact=True, qsc_noise_p1=0.05, qsc_noise_p2=0.1, qsc_readout10=0.05,
                   data_len_for_test=90)
    r = mv.evaluate_snr(10.0, sc, qsc, convs, fc)
    assert calls and all(c is mv.qsc_noise_model() for c in calls)
    assert math.isfinite(r["nmse_quantum"]) and 0.0 <= r["acc_quantum"] <= 1.0
    ql = qsc.qlayer
    assert (ql.shots, ql.noise, ql.exact_noise) == (None, None, False)   # the layer is handed back as it was
    n_calls = len(calls)
    r2 = mv.evaluate_snr(10.0, sc, qsc, convs, fc)   # no Monte-Carlo: the same numbers
    assert r2 == r and len(calls) == 2 * n_calls
    plain = model_val(device="cpu", data_len_for_test=90).evaluate_snr(10.0, sc, qsc, convs, fc)
    assert len(calls) == 2 * n_calls and plain["nmse_classical"] == r["nmse_classical"]


# ------------------------------------------------------------------------------- refusals
def test_rejected_arguments():
    x, w = inputs(4, 2, 3)
    gE = torch.ones(3, 4)
    for f in (lambda **kw: qsim_mixed(x, w, **kw), lambda **kw: qsim_mixed_probs(x, w, **kw),
              lambda **kw: mixed_rows(x, w, gE, **kw)):
        with pytest.raises(ValueError, match="NoiseModel"):
            f(noise=None, backend="cpu")
        with pytest.raises(ValueError, match="NoiseModel"):
            f(noise=0.01, backend="cpu")
        with pytest.raises(ValueError, match="torch"):
            f(noise=NOISE, backend="torch")
        with pytest.raises(ValueError, match="unknown backend"):
            f(noise=NOISE, backend="cuda")
        with pytest.raises(ValueError, match="CUDA tensors"):   # CPU tensors on the hip backend
            f(noise=NOISE, backend="hip")
        f(noise=NoiseModel(), backend="cpu")   # all rates zero: allowed
    x9, w9 = inputs(9, 1, 1)
    assert MIXED_MAX_QUBITS == 8
    with pytest.raises(NotImplementedError, match="8"):
        qsim_mixed(x9, w9, NOISE, "cpu")
    with pytest.raises(NotImplementedError, match="8"):
        mixed_rows(x9, w9, torch.ones(1, 9), NOISE, "cpu")
    with pytest.raises(ValueError):   # n = 1: the ring needs two wires
        qsim_mixed(torch.zeros(1, 1), torch.zeros(1, 1, 2), NOISE, "cpu")
    with pytest.raises(ValueError, match="4096"):
        qsim_mixed(torch.zeros(1, 2), torch.zeros(1025, 2, 2), NOISE, "cpu")
    with pytest.raises(ValueError, match="gE"):
        mixed_rows(x, w, torch.ones(3, 5), NOISE, "cpu")
    with pytest.raises(ValueError):   # 3 rates for 4 wires
        qsim_mixed(x, w, NoiseModel(p1=[0.1, 0.1, 0.1]), "cpu")
    with pytest.raises(ValueError, match="noise needs shots"):   # qsim itself is as it was
        qsim(x, w, "cpu", noise=NOISE)


# ------------------------------------------------------------------------------- sanitizer driver
@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_mixed_driver_asan_ubsan(tmp_path):
    exe = tmp_path / "qsim_mixed_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", os.path.join(CPU, "qsim_cpu.cpp"),
           os.path.join(CPU, "tests", "qsim_mixed_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
