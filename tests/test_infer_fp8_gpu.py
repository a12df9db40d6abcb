"""The e4m3 test-time estimator (train/infer.py HIPInference(dtype="fp8")) on a real MI355X: the row-quantising
BN + ReLU apply (csrc/hip/conv.hip qd_bn_relu_rows_f8), the estimates against a float64 reference built from the
engine's own e4m3 operands, their independence of chunking and neighbours, and the sweep's ``dtype`` knob.

Setup: the models of tests/test_infer_gpu.py::_models with the last BN bias of expert 2 at -1e3, so every FC-operand
row (sample, 2) is all zero after the ReLU (the zero-row rule: scale 1, zero bytes, and an estimate that is the bias
itself).  The engine runs chunks of 144 on N = 300 samples: three chunks, the last one partial.

Bounds.  With the engine's own h8 / rs / W8 / cs / bias as float64 the reference is ref = (h8 W8^T)[r, j] rs[r] cs[j]
+ b[j]; the kernels add the fp32 accumulation of K = 4096 exact products (with the e4m3 MFMA's alignment term), one fma
and the bf16 store: gemm_oracle.bf16_bound(ref, K, S, align), S and align scaled by rs cs -- the GEMM test's bound
(tests/test_gemm_rows_f8_gpu.py); the mixed estimate has K' = K + E as there.
"""
import pytest
import torch

import gemm_oracle as go
from test_infer_gpu import _models
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import NMSELoss
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import (SCALE_EXP_MAX, SCALE_EXP_MIN,
                                                                                        fp8_linear)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference

pytestmark = pytest.mark.gpu

D, F32, BF, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
N, CHUNK, NE, K = 300, 144, 3, 4096


@pytest.fixture(scope="module")
def setup(cuda):
    convs, fc, sc, qsc = _models(cuda)
    bn3 = [m for m in convs[2].modules() if isinstance(m, torch.nn.BatchNorm2d)][2]
    bn3.bias.data.fill_(-1e3)
    torch.manual_seed(3)
    x = torch.randn(N, 2, 16, 8, device=cuda)
    expert = torch.randint(0, NE, (N,), device=cuda)
    eng = HIPInference(convs, fc, 128, cuda, chunk=CHUNK, dtype="fp8")
    return dict(convs=convs, fc=fc, sc=sc, qsc=qsc, x=x, expert=expert, eng=eng)


def _rows(eng, x, lo):
    """The chunk starting at sample ``lo`` through the experts: (h8 (CHUNK E, K) e4m3, rs (CHUNK E,)) clones."""
    eng._load(x, lo, min(CHUNK, x.shape[0] - lo))
    h8 = eng.conv.forward(eng.x1, training=False)
    return h8.clone(), eng.conv.rs.clone()


# ================================================================================ 1. the tail kernel
def test_rows_kernel_against_the_bf16_apply(cuda, setup):
    eng, x = setup["eng"], setup["x"]
    ref = HIPInference(setup["convs"], setup["fc"], 128, cuda, chunk=CHUNK)
    ref._load(x, 0, CHUNK)
    h3_ref = ref.conv.forward(ref.x1, training=False).clone()
    _rows(eng, x, 0)                                       # (allocates h8r / rs)
    eng.conv.h8r.view(torch.uint8).fill_(0xFF)
    eng.conv.rs.fill_(float("nan"))
    eng.conv.rows_h3 = torch.full_like(h3_ref, float("nan"))
    try:
        h8, rs = _rows(eng, x, 0)
        h3 = eng.conv.rows_h3.clone()
    finally:
        eng.conv.rows_h3 = None
    torch.cuda.synchronize()
    assert torch.equal(h3.view(torch.int16), h3_ref.view(torch.int16))
    hd, rsd = h3.to(D), rs.to(D)
    mx = hd.amax(1)
    zero = mx == 0
    r2 = torch.arange(CHUNK * NE, device=cuda) % NE == 2
    assert bool(zero[r2].all()) and not bool(zero[~r2].any())
    assert bool((rs[zero] == 1).all())
    assert go.is_pow2(rsd)
    e = torch.log2(rsd).round()
    assert bool(((e >= SCALE_EXP_MIN) & (e <= SCALE_EXP_MAX)).all())
    nz = ~zero
    assert bool((448 * rsd[nz] >= mx[nz]).all()) and bool((mx[nz] > 448 * rsd[nz] / 2).all())
    want = go.round_e4m3(hd / rsd[:, None]).to(F32).to(F8)
    assert torch.equal(h8.view(torch.uint8), want.view(torch.uint8))
    assert bool((h8.view(torch.uint8)[zero] == 0).all())


# ================================================================================ 2. estimates against float64
def _float64_products(setup):
    """Per sample row (i, e): the float64 product of the engine's own operands, its magnitude sum and alignment term,
    scaled by rs cs: (prod, Sabs, align) (N, E, 2048), and the bias (2048,)."""
    if "prods" not in setup:
        eng, x = setup["eng"], setup["x"]
        W = eng.W8.to(F32).to(D)
        cs = eng.cs.to(D)
        out = [[], [], []]
        for lo in range(0, N, CHUNK):
            n = min(CHUNK, N - lo)
            h8, rs = _rows(eng, x, lo)
            h = h8.to(F32).to(D)[:n * NE]
            s = rs.to(D)[:n * NE, None] * cs[None, :]
            for o, t in zip(out, (h @ W.t(), h.abs() @ W.abs().t(), go.e4m3_align(h, W))):
                o.append((t * s).view(n, NE, -1))
        setup["prods"] = tuple(torch.cat(o) for o in out) + (eng.b_lp.to(D),)
    return setup["prods"]


def test_estimate_against_float64(cuda, setup):
    eng, x, expert = setup["eng"], setup["x"], setup["expert"]
    prod, Sabs, align, b = _float64_products(setup)
    pick = lambda t: t[torch.arange(N, device=cuda), expert]
    ref = pick(prod) + b
    H = eng.estimate(x, expert)
    torch.cuda.synchronize()
    assert H.shape == (N, 2048) and H.dtype == F32
    r = go.worst_ratio((H.to(D) - ref).abs(), go.bf16_bound(ref, K, pick(Sabs) + b.abs(), pick(align)))
    print(f"ERRBOUND infer_fp8 estimate {r:.4f}")
    assert r <= 1.0, r
    z = expert == 2
    assert bool(z.any()) and torch.equal(H[z], eng.b_lp.float().expand(int(z.sum()), -1))


def test_estimate_mixed_against_float64(cuda, setup):
    eng, x = setup["eng"], setup["x"]
    prod, Sabs, align, b = _float64_products(setup)
    P = torch.softmax(4 * torch.randn(N, NE, generator=torch.Generator().manual_seed(11)), 1).to(cuda)
    P[5] = 0.0
    Pd = P.to(D)[:, :, None]
    ref = (Pd * prod).sum(1) + b
    S = (Pd.abs() * Sabs).sum(1) + b.abs()
    H = eng.estimate_mixed(x, P)
    torch.cuda.synchronize()
    r = go.worst_ratio((H.to(D) - ref).abs(), go.bf16_bound(ref, K + NE, S, (Pd.abs() * align).sum(1)))
    print(f"ERRBOUND infer_fp8 estimate_mixed {r:.4f}")
    assert r <= 1.0, r
    assert torch.equal(H[5], eng.b_lp.float())


# ================================================================================ 3. independence
def test_estimate_does_not_depend_on_chunk_or_neighbours(cuda, setup):
    eng, x, expert, convs, fc = (setup[k] for k in ("eng", "x", "expert", "convs", "fc"))
    H = eng.estimate(x, expert)
    H288 = HIPInference(convs, fc, 128, cuda, chunk=288, dtype="fp8").estimate(x, expert)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2)).to(cuda)
    Hp = eng.estimate(x[perm], expert[perm])
    torch.cuda.synchronize()
    assert torch.equal(H, H288)
    assert torch.equal(H[perm], Hp)


def test_per_tensor_fp8_linear_depends_on_its_batch(cuda, setup):
    """The trainer's torch ``fp8_linear`` takes ONE activation scale over the batch it is handed, so the same samples
    in chunks of 144 and of 288 give different estimates: the reason for per-row scales."""
    x, expert, convs, fc = (setup[k] for k in ("x", "expert", "convs", "fc"))
    with torch.no_grad():
        feats = torch.stack([c(x[:288]) for c in convs])                      # (E, 288, K)
        a = feats[expert[:288], torch.arange(288, device=cuda)].to(BF)
        w, b = fc.FC.weight.detach(), fc.FC.bias.detach().to(BF)
        y144 = torch.cat([fp8_linear(a[:144], w, b), fp8_linear(a[144:], w, b)])
        y288 = fp8_linear(a, w, b)
    torch.cuda.synchronize()
    assert y144.shape == y288.shape and not torch.equal(y144, y288)


# ================================================================================ 4. one-hot
def test_one_hot_mixed_equals_the_routed_estimate(cuda, setup):
    eng, x, expert = setup["eng"], setup["x"], setup["expert"]
    P = torch.zeros(N, NE, device=cuda)
    P[torch.arange(N, device=cuda), expert] = 1.0
    Hm, Hr = eng.estimate_mixed(x, P), eng.estimate(x, expert)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Hm).all()) and torch.equal(Hm, Hr)


def test_refresh_requantises_and_the_chunk_rule(cuda, setup):
    convs, fc = setup["convs"], setup["fc"]
    with pytest.raises(ValueError):
        HIPInference(convs, fc, 128, cuda, chunk=96, dtype="fp8")
    with pytest.raises(ValueError):
        HIPInference(convs, fc, 128, cuda, chunk=144, dtype="int8")
    import copy
    eng = HIPInference(convs, fc, 128, cuda, chunk=144, dtype="fp8")
    W8, cs = eng.W8.clone(), eng.cs.clone()
    fc2 = copy.deepcopy(fc)
    with torch.no_grad():
        fc2.FC.weight.mul_(3.0)
    eng.refresh(convs, fc2)
    assert not torch.equal(eng.cs, cs)
    eng.refresh(convs, fc)
    assert torch.equal(eng.cs, cs) and torch.equal(eng.W8.view(torch.uint8), W8.view(torch.uint8))


# ================================================================================ 5. the sweep
def test_evaluate_snr_dtype_fp8_on_the_engine(cuda, setup):
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.data.channel import (generate_mixed,
                                                                                             pack_channel, pack_pilots)
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.evaluate import model_val
    convs, fc, sc, qsc = (setup[k] for k in ("convs", "fc", "sc", "qsc"))
    mv = model_val(device="cuda", dtype="fp8", routing="soft", data_len_for_test=600)
    r = mv.evaluate_snr(10.0, sc, qsc, convs, fc)
    rows = {"nmse_ls", "nmse_mmse", "nmse_lmmse", "nmse_classical", "nmse_quantum", "acc_classical", "acc_quantum",
            "nmse_classical_soft", "nmse_quantum_soft", "nmse_oracle"}
    assert set(r) == rows and all(v == v and abs(v) != float("inf") for v in r.values()), r
    eng = mv._eng
    assert eng.dtype == "fp8"
    Yp, _, H, ind = generate_mixed(600, 10.0, 128, mv.indicator, base_seed=mv.seed,
                                   split=f"test@{mv.training_data_len * 3}", device=cuda)
    direct = float(NMSELoss()(eng.estimate(pack_pilots(Yp, 128), ind), pack_channel(H)))
    assert r["nmse_oracle"] == direct
    r2 = mv.evaluate_snr(10.0, sc, qsc, convs, fc)
    assert mv._eng is eng and r2 == r
    mv.dtype = "bf16"
    r3 = mv.evaluate_snr(10.0, sc, qsc, convs, fc)
    assert mv._eng is not eng and mv._eng.dtype == "bf16" and set(r3) == rows


# ================================================================================ 6. fp8 against bf16 (reported)
def test_fp8_against_bf16_is_reported(cuda, setup):
    """No a-priori bound exists for the e4m3 estimate against the bf16 one on real weights (the e4m3 half-ulp of 2^-4
    per operand only suggests a few percent): the value is printed, not asserted."""
    eng, x, expert = setup["eng"], setup["x"], setup["expert"]
    H8 = eng.estimate(x, expert)
    H16 = HIPInference(setup["convs"], setup["fc"], 128, cuda, chunk=CHUNK).estimate(x, expert)
    torch.cuda.synchronize()
    rel = float((H8 - H16).norm() / H16.norm())
    print(f"FP8REL {rel:.4e}")
    assert bool(torch.isfinite(H8).all())
