"""Soft (posterior-weighted) test-time routing on the HIP inference engine (train/infer.py): the mixed estimate against
the routed one and against the torch definition, and the classifiers' log-posteriors.

Small random-init models; the mixed path runs at chunk = 48 with N = 70 samples: two chunks, the last one partial.
(The routed estimate it is compared with bit for bit comes from an engine at chunk = 144, the smallest the routed
GEMM tiles -- a sample's estimate does not depend on its chunk: eval-mode convs and GEMM rows are per sample.)"""
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import (Conv_P128, FC_P128,
                                                                                             QSC_P128, SC_P128)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import estimate_mixed
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference

pytestmark = pytest.mark.gpu

CHUNK, N = 48, 70


@pytest.fixture(scope="module")
def setup(cuda):
    torch.manual_seed(0)
    convs = [Conv_P128(128).to(cuda).eval() for _ in range(3)]
    for c in convs:   # non-trivial running statistics
        for mod in c.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.5, 1.5)
                mod.bias.data.uniform_(-0.1, 0.1)
    fc = FC_P128(128).to(cuda).eval()
    sc = SC_P128(128).to(cuda).eval()
    qsc = QSC_P128(8, 3, 3, False, False, 128).to(cuda).eval()
    eng = HIPInference(convs, fc, 128, cuda, chunk=CHUNK, sc=sc, qsc=qsc)
    x = torch.randn(N, 2, 16, 8, device=cuda)
    return convs, fc, eng, x


def test_one_hot_weights_equal_the_routed_estimate(cuda, setup):
    convs, fc, eng, x = setup
    expert = torch.randint(0, 3, (N,), device=cuda)
    P = torch.zeros(N, 3, device=cuda)
    P[torch.arange(N, device=cuda), expert] = 1.0
    Hm = eng.estimate_mixed(x, P)
    routed = HIPInference(convs, fc, 128, cuda, chunk=144)
    Hr = routed.estimate(x, expert)
    torch.cuda.synchronize()
    assert Hm.shape == Hr.shape == (N, 2048) and bool(torch.isfinite(Hm).all())
    assert torch.equal(Hm, Hr)


def test_posterior_weights_match_the_torch_definition(cuda, setup):
    convs, fc, eng, x = setup
    _, logp = eng.classify(x, "classical", return_logp=True)
    w = logp.exp()
    Hm = eng.estimate_mixed(x, w)
    ref = estimate_mixed(convs, fc, x, w)
    torch.cuda.synchronize()
    err = float((Hm - ref).norm() / ref.norm())
    print(f"soft-routed estimate: relative Frobenius error {err:.3e}")
    assert err < 1e-2, err
    with pytest.raises(ValueError):
        eng.estimate_mixed(x, w[:, :2])


@pytest.mark.parametrize("tag", ["classical", "quantum"])
def test_classify_returns_the_log_posterior_of_its_prediction(cuda, setup, tag):
    _, _, eng, x = setup
    pred0 = eng.classify(x, tag)
    pred, logp = eng.classify(x, tag, return_logp=True)
    torch.cuda.synchronize()
    assert torch.equal(pred, pred0)
    assert logp.shape == (N, 3) and logp.dtype == torch.float32
    assert float(torch.logsumexp(logp, 1).abs().max()) <= 1e-5
    top = logp.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) >= 1e-3
    assert bool(clear.any())
    assert torch.equal(logp.argmax(1)[clear], pred[clear])


def test_measured_log_posterior_follows_the_seed(cuda, setup):
    _, _, eng, x = setup
    p1, l1 = eng.classify(x, "quantum", shots=257, seed=3, return_logp=True)
    p2, l2 = eng.classify(x, "quantum", shots=257, seed=3, return_logp=True)
    p3, l3 = eng.classify(x, "quantum", shots=257, seed=4, return_logp=True)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
    assert not torch.equal(l1, l3)
    assert float(torch.logsumexp(l1, 1).abs().max()) <= 1e-5


def test_evaluate_snr_soft_rows_on_the_engine(cuda, setup):
    """The sweep's GPU path: routing="soft" adds the three rows (engine classify / estimate_mixed / oracle estimate);
    the hard rows are those of routing="hard"."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.evaluate import model_val
    convs, fc, eng, _ = setup
    sc = eng._sc_mod
    hard = model_val(device="cuda", data_len_for_test=300).evaluate_snr(10.0, sc, None, convs, fc)
    soft = model_val(device="cuda", data_len_for_test=300, routing="soft").evaluate_snr(10.0, sc, None, convs, fc)
    assert set(soft) == set(hard) | {"nmse_classical_soft", "nmse_quantum_soft", "nmse_oracle"}
    assert all(soft[k] == hard[k] or (soft[k] != soft[k] and hard[k] != hard[k]) for k in hard)
    assert soft["nmse_classical_soft"] == soft["nmse_classical_soft"] and soft["nmse_oracle"] == soft["nmse_oracle"]
    assert soft["nmse_quantum_soft"] != soft["nmse_quantum_soft"]   # (no quantum classifier: NaN like its hard row)
