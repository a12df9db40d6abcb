"""The density-matrix adjoint on the host (csrc/cpu/qsim_cpu.cpp qd_cpu_qsim_mixed_adjoint; ops/quantum.py
``mixed_adjoint_rows`` / ``qsim_mixed(diff_method="adjoint")`` on ``cpu``): the complex128 twin against the float64
shift rule -- existing code that shares nothing with it -- per entry, the autograd path, the refusals, the layer's and
the runner's knobs, and the sanitizer driver.

The bound is tests/test_mixed_adjoint_gpu.py's formula with eps = 2^-53 and tau = 2^-52 (libm's sin and cos); its
reference term, the shift rule's fp32 angles and fp32 result, (2^-22 + 2^-24) sum |gE|, is what remains."""
import math
import os
import shutil
import subprocess
import warnings

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.config import RunnerConfig
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QuantumLayer
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import quantum as Q
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import (NoiseModel, mixed_adjoint_rows,
                                                                                         mixed_rows, qsim_mixed)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.runner import Y2HRunner
from test_mixed_adjoint_gpu import CASES, README_CASE, OverHalf, amplification, bound, inputs, oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "quantum_distributed_machine_learning_ris_channel_estimation_amd", "csrc", "cpu")
NOISE = NoiseModel(p1=0.02, p2=0.05, readout01=0.02, readout10=0.03)


# ------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("kind", ["mild", "half"])
@pytest.mark.parametrize("n,L,B,G", CASES)
def test_twin_against_the_shift_rule(n, L, B, G, kind):
    twin_check(n, L, B, G, kind)


def test_twin_at_the_readme_noise_point():
    twin_check(*README_CASE, "readme")


def twin_check(n, L, B, G, kind):
    x, w, _ = inputs(n, L, B, G)
    noise, gE, ref = oracle(n, L, B, G, kind)
    got = Q._mixed_adjoint_cpu(x, w, gE, noise)
    assert got.dtype == torch.float64 and got.shape == (B, 2 * n * L)
    bd = bound(n, L, noise, gE, eps=2.0 ** -53, tau=2.0 ** -52)
    err = (got - ref).abs()
    print(f"host twin {kind} n={n} L={L} B={B} G={G}: A = {amplification(noise, n, L):.3g}, worst |dG| = "
          f"{float(err.max()):.3e}, bound {float(bd.min()):.3e} .. {float(bd.max()):.3e}, max |G| = "
          f"{float(ref.abs().max()):.3e}")
    assert bool((err <= bd).all())
    if kind != "half":
        assert float(ref.abs().max(1).values.min()) > 10 * float(bd.max())
    assert torch.equal(mixed_adjoint_rows(x, w, gE, noise, "cpu"), got.float())   # the public function, fp32


# ------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("n,L,B,G", [(3, 2, 5, 0), (6, 2, 3, 3)])
def test_autograd_is_the_rows(n, L, B, G):
    x, w, _ = inputs(n, L, B, G)
    noise, gE, _ = oracle(n, L, B, G, "half")
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    E = qsim_mixed(xa, wa, noise, "cpu", diff_method="adjoint")
    (E * gE).sum().backward()
    dx, dw = Q._rows_to_grads(mixed_adjoint_rows(x, w, gE, noise, "cpu"), x, w, "cpu")
    assert torch.equal(E.detach(), qsim_mixed(x, w, noise, "cpu"))
    assert torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw) and wa.grad.shape == w.shape
    # the default is the shift rule, as before
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    (qsim_mixed(xs, ws, noise, "cpu") * gE).sum().backward()
    dx0, dw0 = Q._rows_to_grads(mixed_rows(x, w, gE, noise, "cpu"), x, w, "cpu")
    assert torch.equal(xs.grad, dx0) and torch.equal(ws.grad, dw0)
    assert float((xs.grad - xa.grad).abs().max()) < 1e-5 and not torch.equal(ws.grad, wa.grad)


def test_quantum_layer_exact_diff_method():
    torch.manual_seed(0)
    layer = QuantumLayer(4, 2, backend="cpu", noise=NOISE)
    assert layer.exact_diff_method == "parameter_shift"
    layer.exact_noise = True
    x = torch.rand(3, 4) * 2 - 1
    grads = {}
    for dm in ("parameter_shift", "adjoint"):
        layer.exact_diff_method = dm
        layer.weights.grad = None
        xa = x.clone().requires_grad_()
        E = layer(xa)
        E.square().sum().backward()
        grads[dm] = (E.detach().clone(), xa.grad.clone(), layer.weights.grad.clone())
    gE = 2 * grads["adjoint"][0]
    G = mixed_adjoint_rows(x, layer.weights.detach(), gE, NOISE, "cpu")
    assert torch.equal(grads["adjoint"][0], grads["parameter_shift"][0])
    assert torch.equal(grads["adjoint"][1], G[:, 0:8:2]) and torch.equal(grads["adjoint"][2].reshape(-1), G.sum(0))
    assert float((grads["adjoint"][2] - grads["parameter_shift"][2]).abs().max()) < 1e-5
    layer.exact_diff_method = "backprop"
    with pytest.raises(ValueError, match="diff_method"):
        layer(x)


# ------------------------------------------------------------------------------- refusals
def test_rejected_arguments():
    x, w = torch.zeros(3, 4), torch.zeros(2, 4, 2)
    gE = torch.ones(3, 4)
    for bad in (OverHalf(1, p1=0.1), OverHalf(2, p2=0.5)):
        with pytest.raises(ValueError, match="parameter_shift"):
            mixed_adjoint_rows(x, w, gE, bad, "cpu")
        with pytest.raises(ValueError, match="parameter_shift"):
            qsim_mixed(x, w, bad, "cpu", diff_method="adjoint")
        assert qsim_mixed(x, w, bad, "cpu").shape == (3, 4)   # the shift rule's path takes them
    assert mixed_adjoint_rows(x, w, gE, NoiseModel(p1=0.5, p2=0.5), "cpu").shape == (3, 16)   # exactly 0.5 is admitted
    with pytest.raises(ValueError, match="diff_method"):
        qsim_mixed(x, w, NOISE, "cpu", diff_method="backprop")
    with pytest.raises(NotImplementedError, match="8"):
        mixed_adjoint_rows(torch.zeros(2, 9), torch.zeros(1, 9, 2), torch.ones(2, 9), NOISE, "cpu")
    with pytest.raises(ValueError, match="gE must be"):
        mixed_adjoint_rows(x, w, torch.ones(3, 5), NOISE, "cpu")
    with pytest.raises(ValueError, match="gE must be on"):
        mixed_adjoint_rows(x, w, torch.ones(3, 4, device="meta"), NOISE, "cpu")
    with pytest.raises(ValueError, match="NoiseModel"):
        mixed_adjoint_rows(x, w, gE, None, "cpu")
    with pytest.raises(ValueError, match="torch backend"):
        mixed_adjoint_rows(x, w, gE, NOISE, "torch")


# ------------------------------------------------------------------------------- the runner's knobs
def _runner(tmp_path, name, **knobs):
    return Y2HRunner(n_epochs=2, data_len=60, batch_size_DML=16, device="cpu", workspace=str(tmp_path / name),
                     data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2, use_quantumnat=True,
                     seed=0, qsc_noise_p1=0.02, qsc_noise_p2=0.05, qsc_readout01=0.02, qsc_readout10=0.03, **knobs)


def test_runner_knobs(tmp_path, monkeypatch):
    assert RunnerConfig().qsc_noise_exact is False
    for s, v in (("true", True), ("1", True), ("false", False), ("0", False)):
        assert RunnerConfig().update_from_dict({"qsc_noise_exact": s}).qsc_noise_exact is v
    with pytest.raises(ValueError, match="needs qsc_shots == 0"):
        _runner(tmp_path, "a", qsc_noise_exact=True, qsc_shots=64).qsc_device_knobs()
    with pytest.raises(ValueError, match="need qsc_shots > 0"):   # without the flag: today's message
        _runner(tmp_path, "b").qsc_device_knobs()
    with pytest.raises(ValueError, match="qsc_diff_method=adjoint"):
        _runner(tmp_path, "c", qsc_noise_exact=True, qsc_diff_method="parameter_shift").qsc_device_knobs()
    with pytest.raises(ValueError, match="n_qubits <= 8"):
        Y2HRunner(device="cpu", workspace=str(tmp_path / "d"), data_dir=str(tmp_path / "data"), n_qubits=9,
                  qsc_noise_p1=0.01, qsc_noise_exact=True).qsc_device_knobs()
    with pytest.raises(ValueError, match=r"\[0, 0.5\]"):   # (NoiseModel admits no larger rate)
        Y2HRunner(device="cpu", workspace=str(tmp_path / "e"), data_dir=str(tmp_path / "data"), n_qubits=4,
                  qsc_noise_p1=0.6, qsc_noise_exact=True).qsc_device_knobs()
    k = _runner(tmp_path, "f", qsc_noise_exact=True).qsc_device_knobs()
    assert k["exact_noise"] is True and k["shots"] is None and k["diff_method"] == "adjoint"
    assert isinstance(k["noise"], NoiseModel)
    # the flag without a rate changes nothing
    assert Y2HRunner(device="cpu", workspace=str(tmp_path / "g"), data_dir=str(tmp_path / "data"),
                     qsc_noise_exact=True).qsc_device_knobs() is None
    r = _runner(tmp_path, "h", qsc_noise_exact=True)
    monkeypatch.setattr(r._context(), "world", 2)   # (restored: the context outlives the runner)
    with pytest.raises(ValueError, match="world size 1"):
        r.qsc_device_knobs()


def test_train_qsc_against_the_exact_channel(tmp_path):
    r = _runner(tmp_path, "w", qsc_noise_exact=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = r.train_QSC_P128()
    assert m.qlayer.exact_noise is True and m.qlayer.exact_diff_method == "adjoint" and not m.qlayer.shots
    assert len(r.train_QSC_losses) == 2 and all(math.isfinite(v) for v in r.train_QSC_losses)
    assert all(math.isfinite(v) for v in r.val_QSC_losses)   # validated under the same channel
    assert float(m.qlayer.weights.grad.abs().max()) > 0


# ------------------------------------------------------------------------------- sanitizer driver
@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_mixed_adjoint_driver_asan_ubsan(tmp_path):
    exe = tmp_path / "qsim_mixed_adjoint_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", os.path.join(CPU, "qsim_cpu.cpp"),
           os.path.join(CPU, "tests", "qsim_mixed_adjoint_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qsim_mixed_adjoint_check: 0 failures" in r.stdout
