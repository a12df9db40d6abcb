"""Soft (posterior-weighted) test-time routing on the CPU: the torch definition ``engine.estimate_mixed`` and the
sweep's ``routing`` option (train/evaluate.py) on tiny untrained models."""
import math

import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.config import EvalConfig
from quantum_distributed_machine_learning_ris_channel_estimation_amd.data.channel import generate_mixed
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                             SC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import (estimate_mixed,
                                                                                        estimate_routed)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.evaluate import model_val

HARD_KEYS = {"nmse_ls", "nmse_mmse", "nmse_lmmse", "nmse_classical", "nmse_quantum", "acc_classical", "acc_quantum"}
SOFT_KEYS = {"nmse_classical_soft", "nmse_quantum_soft", "nmse_oracle"}
NTEST = 300   # (the smallest data_len_for_test of tests/test_evaluate_cpu.py)


def _models():
    torch.manual_seed(0)
    convs = [Conv_P128(128).eval() for _ in range(3)]
    return SC_P128(128).eval(), convs, FC_P128(128).eval()


class Fixed(SC_P128):
    """A classifier whose posterior is one-hot to fp32: zero weights and a final bias of +50 on the wanted class,
    -50 on the others -- ``labels`` in call order (None: class ``const`` for every sample)."""

    def __init__(self, labels=None, const=0):
        super().__init__(128)
        self.labels, self.const, self.at = labels, const, 0

    def forward(self, x):
        n = x.shape[0]
        lab = torch.full((n,), self.const) if self.labels is None else self.labels[self.at:self.at + n]
        self.at += n
        logits = torch.full((n, 3), -50.0)
        logits[torch.arange(n), lab] = 50.0
        return torch.log_softmax(logits, 1)


# ------------------------------------------------------------------------------------------ estimate_mixed
def test_estimate_mixed_one_hot_is_estimate_routed():
    _, convs, fc = _models()
    x = torch.randn(40, 2, 16, 8)
    expert = torch.arange(40) % 3
    w = torch.zeros(40, 3)
    w[torch.arange(40), expert] = 1.0
    assert torch.allclose(estimate_mixed(convs, fc, x, w, chunk=16), estimate_routed(convs, fc, x, expert),
                          rtol=1e-6, atol=1e-6)


def test_estimate_mixed_is_linear_in_the_weights():
    _, convs, fc = _models()
    x = torch.randn(24, 2, 16, 8)
    a, b = torch.rand(24, 3), torch.rand(24, 3)
    lhs = estimate_mixed(convs, fc, x, 2.0 * a - 0.5 * b)
    rhs = 2.0 * estimate_mixed(convs, fc, x, a) - 0.5 * estimate_mixed(convs, fc, x, b)
    assert torch.allclose(lhs, rhs, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(24, 2), (23, 3), (24, 3, 1), (72,)])
def test_estimate_mixed_refuses_a_wrong_weight_shape(shape):
    _, convs, fc = _models()
    with pytest.raises(ValueError):
        estimate_mixed(convs, fc, torch.randn(24, 2, 16, 8), torch.rand(*shape))


# ------------------------------------------------------------------------------------------ the sweep
def test_routing_hard_returns_the_former_keys_and_soft_adds_three():
    sc, convs, fc = _models()
    assert EvalConfig().routing == "hard"
    hard = model_val(device="cpu", data_len_for_test=NTEST).evaluate_snr(10.0, sc, None, convs, fc)
    assert set(hard) == HARD_KEYS
    soft = model_val(device="cpu", data_len_for_test=NTEST, routing="soft").evaluate_snr(10.0, sc, None, convs, fc)
    assert set(soft) == HARD_KEYS | SOFT_KEYS
    for k in HARD_KEYS:   # the hard rows do not move
        assert soft[k] == hard[k] or (math.isnan(soft[k]) and math.isnan(hard[k])), k
    assert all(math.isfinite(soft[k]) for k in ("nmse_classical_soft", "nmse_oracle"))
    assert math.isnan(soft["nmse_quantum_soft"])   # (no quantum classifier: NaN, like its hard row)
    # with both classifiers every new row is finite (the "quantum" slot takes any scenario classifier)
    both = model_val(device="cpu", data_len_for_test=NTEST, routing="soft").evaluate_snr(10.0, sc, SC_P128(128).eval(),
                                                                                      convs, fc)
    assert set(both) == HARD_KEYS | SOFT_KEYS and all(math.isfinite(both[k]) for k in SOFT_KEYS)


def test_one_hot_posterior_makes_the_soft_row_the_hard_row():
    _, convs, fc = _models()
    r = model_val(device="cpu", data_len_for_test=NTEST, routing="soft").evaluate_snr(10.0, Fixed(const=1), None,
                                                                                   convs, fc)
    assert math.isclose(r["nmse_classical_soft"], r["nmse_classical"], rel_tol=1e-5)


def test_oracle_row_is_the_hard_row_of_a_classifier_that_is_always_right():
    _, convs, fc = _models()
    mv = model_val(device="cpu", data_len_for_test=NTEST, routing="soft")
    ind = generate_mixed(NTEST, 10.0, mv.Pilot_num, mv.indicator, base_seed=mv.seed,
                         split=f"test@{mv.training_data_len * 3}", device=mv.device)[3]
    r = mv.evaluate_snr(10.0, Fixed(labels=ind.long()), None, convs, fc)
    assert r["acc_classical"] == 1.0
    assert math.isclose(r["nmse_oracle"], r["nmse_classical"], rel_tol=1e-6)
    assert math.isclose(r["nmse_classical_soft"], r["nmse_classical"], rel_tol=1e-5)


def test_unknown_routing_and_class_count_are_value_errors():
    sc, convs, fc = _models()
    with pytest.raises(ValueError):
        model_val(device="cpu", data_len_for_test=NTEST, routing="x")
    with pytest.raises(ValueError):
        model_val(device="cpu", data_len_for_test=NTEST, routing="soft").evaluate_snr(10.0, SC_P128(128, 4).eval(),
                                                                                   None, convs, fc)
