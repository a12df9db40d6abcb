"""The torch definition of the e4m3 test-time estimator (train/engine.py: scale_exponent, quantise_rows_e4m3, the
``dtype="fp8"`` estimates) and the sweep's ``dtype`` knob, on the CPU."""
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.config import EvalConfig
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import Conv_P128, FC_P128, SC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train import engine
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import (estimate_mixed, estimate_routed,
                                                                                        quantise_rows_e4m3,
                                                                                        scale_exponent)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.evaluate import model_val

F32 = torch.float32


def _next(v: float) -> float:
    return float(torch.nextafter(torch.tensor(v, dtype=F32), torch.tensor(float("inf"), dtype=F32)))


def test_scale_exponent():
    se = lambda *v: scale_exponent(torch.tensor(v, dtype=F32)).tolist()
    # exact powers of two: 2^k <= 448 2^e  <=>  e >= k - log2(448), i.e. e = k - 8
    assert se(1.0, 2.0, 256.0, 512.0, 2.0 ** -20, 2.0 ** 20) == [-8, -7, 0, 1, -28, 12]
    # 448 2^k is the largest value of exponent k; the next float above it needs k + 1
    for k in (-10, -1, 0, 1, 7):
        m = 448.0 * 2.0 ** k
        assert se(m, _next(m)) == [k, k + 1], k
    assert se(0.0) == [0]
    # the clamp limits: 448 2^32 and 448 2^-32 are reached exactly, values beyond them keep the limit
    assert se(448.0 * 2.0 ** 32, _next(448.0 * 2.0 ** 32), 1e38, float("inf")) == [32, 32, 32, 32]
    assert se(448.0 * 2.0 ** -32, 448.0 * 2.0 ** -33, 1e-38, 1e-45) == [-32, -32, -32, -32]
    assert scale_exponent(torch.zeros(2, 3)).shape == (2, 3) and scale_exponent(torch.zeros(2)).dtype == torch.int32


def test_quantise_rows_round_trip():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(64, 512, generator=g) * torch.logspace(-6, 6, 64, base=2.0)[:, None]
    h[7] = 0.0
    h[9, 3] = 448.0 * 4                                  # (the row maximum lands on 448 exactly)
    h8, s = quantise_rows_e4m3(h)
    assert h8.dtype == torch.float8_e4m3fn and s.dtype == F32 and s.shape == (64,)
    e = torch.log2(s)
    assert torch.equal(e, e.round()) and s[7] == 1 and bool((h8[7].view(torch.uint8) == 0).all())
    mx = h.abs().amax(1)
    nz = mx > 0
    assert bool((448 * s[nz] >= mx[nz]).all()) and bool((448 * s[nz] / 2 < mx[nz]).all())
    back = h8.float() * s[:, None]
    assert float(back[9, 3]) == 448.0 * 4
    # elements at or above the row's normal range (2^-6 in scaled units): half an e4m3 ulp, 2^-4 relative
    normal = h.abs() >= 2.0 ** -6 * s[:, None]
    rel = ((back - h).abs() / h.abs().clamp_min(1e-30))[normal]
    assert bool(normal.any()) and float(rel.max()) <= 2.0 ** -4
    # below it: the subnormal spacing 2^-9 (scaled), half of it
    assert float(((back - h).abs() / s[:, None])[~normal].max()) <= 2.0 ** -10


def _models():
    torch.manual_seed(0)
    convs = [Conv_P128(128).eval() for _ in range(3)]
    for c in convs:
        for mod in c.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
    return convs, FC_P128(128).eval()


def test_routed_and_mixed_fp8_agree_for_one_hot_weights():
    convs, fc = _models()
    N = 24
    x = torch.randn(N, 2, 16, 8)
    expert = torch.arange(N) % 3
    P = torch.zeros(N, 3)
    P[torch.arange(N), expert] = 1.0
    Hr = estimate_routed(convs, fc, x, expert, dtype="fp8")
    Hm = estimate_mixed(convs, fc, x, P, dtype="fp8")
    assert Hr.dtype == F32 and Hr.shape == (N, 2048) and bool(torch.isfinite(Hr).all())
    assert torch.equal(Hr, Hm)
    # e4m3 is a different model from the fp32 default, and the keyword defaults to today's behaviour
    H32 = estimate_routed(convs, fc, x, expert)
    rel = float((Hr - H32).norm() / H32.norm())
    assert rel > 0, rel
    assert torch.equal(H32, estimate_routed(convs, fc, x, expert, dtype="bf16"))
    with pytest.raises(ValueError):
        estimate_routed(convs, fc, x, expert, dtype="int8")
    with pytest.raises(ValueError):
        estimate_mixed(convs, fc, x, P, dtype="int8")


def test_fp8_definition_does_not_call_scaled_mm(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch._scaled_mm called")
    monkeypatch.setattr(torch, "_scaled_mm", refuse)
    convs, fc = _models()
    x = torch.randn(6, 2, 16, 8)
    estimate_routed(convs, fc, x, torch.arange(6) % 3, dtype="fp8")
    estimate_mixed(convs, fc, x, torch.full((6, 3), 1 / 3), dtype="fp8")


def test_eval_config_dtype_is_validated():
    assert EvalConfig().dtype == "bf16"
    assert model_val(device="cpu", dtype="fp8").dtype == "fp8"
    with pytest.raises(ValueError):
        model_val(EvalConfig(dtype="int8"), device="cpu")
    with pytest.raises(ValueError):
        model_val(device="cpu", dtype="fp16")


def test_evaluate_snr_fp8_runs_the_torch_definition_on_the_cpu(monkeypatch):
    convs, fc = _models()
    sc = SC_P128(128).eval()
    calls = []
    real = engine.quantise_rows_e4m3
    monkeypatch.setattr(engine, "quantise_rows_e4m3", lambda h: (calls.append(tuple(h.shape)), real(h))[1])
    r8 = model_val(device="cpu", data_len_for_test=60, dtype="fp8", routing="soft").evaluate_snr(10.0, sc, None, convs, fc)
    assert calls, "dtype='fp8' did not reach the torch definition"
    n = len(calls)
    r16 = model_val(device="cpu", data_len_for_test=60, routing="soft").evaluate_snr(10.0, sc, None, convs, fc)
    assert len(calls) == n, "the default dtype quantised something"
    assert set(r8) == set(r16)
    for k in ("nmse_classical", "nmse_classical_soft", "nmse_oracle"):
        assert r8[k] == r8[k] and r8[k] != r16[k], k
    for k in ("nmse_ls", "nmse_mmse", "acc_classical"):
        assert r8[k] == r16[k]
