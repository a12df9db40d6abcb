"""The low-latency estimate path (train/infer.py HIPInference.session / InferSession) on a real MI355X: one request of
1..16 samples from pilots to channel as one captured graph -- input packing, classifier, routing on the device, the
experts, and the skinny FC (csrc/hip/gemm_skinny.hip).

Setup: tests/test_infer_gpu.py::_models (pilot 128: random-init Conv_P128 x 3 with non-trivial BN statistics, FC_P128,
SC_P128, an 8-qubit QSC_P128), fixed seeds.  The reference engines run chunks of 48 (bf16) and 144 (fp8): what the
parent offers for the same request, padded with copies of sample 0.  ``batch`` in {1, 5, 16}.

Bounds: the FC of the session against float64 on the session's OWN expert feature rows (checked bit for bit against
the engine's first): gemm_oracle.bf16_bound(ref, K, S[, align]) with K = 4096, the mix K + 3 -- tests/test_gemm_skinny_gpu.py.
"""
import pytest
import torch

import gemm_oracle as go
from test_infer_gpu import _models
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import Conv_P128, FC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.infer import HIPInference

pytestmark = pytest.mark.gpu

D, F32, BF, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
NE, K, NOUT = 3, 4096, 2048
BATCHES = (1, 5, 16)
CHUNK = {"bf16": 48, "fp8": 144}


@pytest.fixture(scope="module")
def setup(cuda):
    convs, fc, sc, qsc = _models(cuda)
    torch.manual_seed(5)
    x = torch.randn(64, 2, 16, 8, device=cuda)
    eng = {dt: HIPInference(convs, fc, 128, cuda, chunk=CHUNK[dt], sc=sc, qsc=qsc, dtype=dt) for dt in ("bf16", "fp8")}
    return dict(convs=convs, fc=fc, sc=sc, qsc=qsc, x=x, eng=eng)


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _out(res):
    """Clones of a run's views (valid until the next run only)."""
    return tuple(None if t is None else t.clone() for t in res)


# ================================================================================ 1. classifier outputs
@pytest.mark.parametrize("which,shots", [("classical", 0), ("quantum", 0), ("quantum", 257)],
                         ids=["classical", "quantum", "quantum-shots257"])
def test_pred_and_logp_equal_the_engines_classify(cuda, setup, which, shots):
    """Bit for bit against ``classify`` on the same samples.  With shots the session's run r reads counter r, the
    engine's chunk r: run 0 is compared with the request alone (chunk 0), run 1 with the request placed at the head
    of chunk 1."""
    eng, x = setup["eng"]["bf16"], setup["x"]
    for batch in BATCHES:
        s = eng.session(batch, which=which, shots=shots, seed=9)
        _, pred, logp = _out(s.run(x[:batch]))
        p_ref, l_ref = eng.classify(x[:batch], which, shots=shots, seed=9, return_logp=True)
        torch.cuda.synchronize()
        assert pred.dtype == torch.int64 and logp.dtype == F32 and logp.shape == (batch, 3)
        assert torch.equal(pred, p_ref), (which, shots, batch)
        assert _same(logp, l_ref), (which, shots, batch, float((logp - l_ref).abs().max()))
        assert torch.equal(pred, logp.argmax(1))
        if shots:
            _, pred1, logp1 = _out(s.run(x[:batch]))
            two = torch.cat([x[16:16 + CHUNK["bf16"]], x[:batch]])
            p2, l2 = eng.classify(two, which, shots=shots, seed=9, return_logp=True)
            torch.cuda.synchronize()
            assert _same(logp1, l2[CHUNK["bf16"]:]) and torch.equal(pred1, p2[CHUNK["bf16"]:])
        s.close()


# ================================================================================ 2. estimate
def _engine_rows(eng, x, batch):
    """The engine's expert feature rows (batch E, K) of x[:batch] (and their scales, fp8)."""
    eng._load(x, 0, batch)
    h = eng.conv.forward(eng.x1, training=False)
    rs = eng.conv.rs[:batch * NE].clone() if eng.dtype == "fp8" else None
    return h[:batch * NE].clone(), rs


@pytest.mark.parametrize("routing", ["hard", "soft"])
@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_rows_equal_the_engines_and_h_is_within_the_fc_bound(cuda, setup, dt, routing):
    eng, x = setup["eng"][dt], setup["x"]
    fails = []
    for batch in BATCHES:
        g = torch.Generator().manual_seed(40 + batch)
        expert = torch.randint(0, NE, (batch,), generator=g).to(cuda)
        P = torch.softmax(3 * torch.randn(batch, NE, generator=g), 1).to(cuda)
        s = eng.session(batch, which=None, routing=routing)
        res = s.run(x[:batch], expert=expert) if routing == "hard" else s.run(x[:batch], weights=P)
        H = res[0].clone()
        assert res[2] is None and H.shape == (batch, NOUT) and H.dtype == BF
        torch.cuda.synchronize()
        h_ref, rs_ref = _engine_rows(eng, x, batch)
        if dt == "fp8":
            h, rs = s.conv.h8r.clone(), s.conv.rs.clone()
            assert _same(h, h_ref) and _same(rs, rs_ref), (dt, batch)
            W, sc = eng.W8.to(F32).to(D), rs.to(D)[:, None] * eng.cs.to(D)[None, :]
            hd = h.to(F32).to(D)
            align = go.e4m3_align(hd, W) * sc
        else:
            h = s.conv.h3.clone()
            assert _same(h, h_ref), (dt, batch)
            W, hd = eng.W_lp.to(D), h.to(D)
            sc = torch.ones(batch * NE, NOUT, dtype=D, device=cuda)
            align = torch.zeros(batch * NE, NOUT, dtype=D, device=cuda)
        b = eng.b_lp.to(D)
        v3 = lambda t: t.view(batch, NE, NOUT)
        prod, Sabs, align = v3((hd @ W.t()) * sc), v3((hd.abs() @ W.abs().t()) * sc), v3(align)
        if routing == "hard":
            pick = lambda t: t[torch.arange(batch, device=cuda), expert]
            ref, S, al, Kb = pick(prod) + b, pick(Sabs) + b.abs(), pick(align), K
        else:
            Pd = P.to(D)[:, :, None]
            ref, S, al, Kb = (Pd * prod).sum(1) + b, (Pd.abs() * Sabs).sum(1) + b.abs(), (Pd.abs() * align).sum(1), K + NE
        r = go.worst_ratio((H.to(D) - ref).abs(), go.bf16_bound(ref, Kb, S, al))
        print(f"ERRBOUND session {dt} {routing} batch{batch} {r:.4f}")
        if not r <= 1.0:
            fails.append(f"{dt} {routing} batch {batch}: max err / bound = {r}")
        s.close()
    assert not fails, "\n".join(fails)


# ================================================================================ 3. routing on the device
@pytest.mark.parametrize("routing", ["hard", "soft"])
@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_device_routing_equals_a_session_fed_the_classifiers_output(cuda, setup, dt, routing):
    eng, x = setup["eng"][dt], setup["x"]
    for batch in (5, 16):
        s = eng.session(batch, which="quantum", routing=routing)
        H, pred, logp = _out(s.run(x[:batch]))
        s0 = eng.session(batch, which=None, routing=routing)
        if routing == "hard":
            H0 = s0.run(x[:batch], expert=pred)[0].clone()
        else:
            H0 = s0.run(x[:batch], weights=torch.exp(logp))[0].clone()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(H.float()).any()) and _same(H, H0), (dt, routing, batch)
        s.close()
        s0.close()


# ================================================================================ 4. replays
@pytest.mark.parametrize("dt,which,routing", [("bf16", "quantum", "hard"), ("fp8", "classical", "soft")])
def test_three_inputs_through_one_session_equal_fresh_sessions(cuda, setup, dt, which, routing):
    eng, x = setup["eng"][dt], setup["x"]
    batch = 5
    s = eng.session(batch, which=which, routing=routing)
    for k in range(3):
        xs = x[7 * k:7 * k + batch]
        got = _out(s.run(xs))
        f = eng.session(batch, which=which, routing=routing)
        want = _out(f.run(xs))
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(got, want)), k
        f.close()
    s.close()


def test_shots_runs_draw_fresh_streams_that_a_fresh_session_reproduces(cuda, setup):
    eng, x = setup["eng"]["bf16"], setup["x"]
    batch = 16
    runs = []
    for _ in range(2):
        s = eng.session(batch, which="quantum", shots=257, seed=3)
        runs.append([_out(s.run(x[:batch])) for _ in range(2)])
        s.close()
    torch.cuda.synchronize()
    assert not _same(runs[0][0][2], runs[0][1][2]), "two runs drew the same shots"
    for r in range(2):
        assert all(_same(a, b) for a, b in zip(runs[0][r], runs[1][r])), r
    other = eng.session(batch, which="quantum", shots=257, seed=4)
    assert not _same(_out(other.run(x[:batch]))[2], runs[0][0][2])
    other.close()


# ================================================================================ 5. shared weights
def _new_models(cuda):
    torch.manual_seed(77)
    convs = [Conv_P128(128).to(cuda).eval() for _ in range(3)]
    for c in convs:
        for mod in c.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.3, 0.3)
                mod.running_var.uniform_(0.4, 1.5)
    return convs, FC_P128(128).to(cuda).eval()


@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_refresh_and_load_bn_stats_reach_the_session(cuda, setup, dt):
    x, batch = setup["x"], 5
    mk = lambda convs, fc: HIPInference(convs, fc, 128, cuda, chunk=CHUNK[dt], sc=setup["sc"], dtype=dt)
    eng = mk(setup["convs"], setup["fc"])
    s = eng.session(batch, which="classical", routing="soft")
    before = _out(s.run(x[:batch]))
    convs2, fc2 = _new_models(cuda)
    eng.refresh(convs2, fc2)
    after = _out(s.run(x[:batch]))
    want = _out(mk(convs2, fc2).session(batch, which="classical", routing="soft").run(x[:batch]))
    torch.cuda.synchronize()
    assert not _same(before[0], after[0])
    assert all(_same(a, b) for a, b in zip(after, want))
    # BN statistics alone
    convs3, _ = _new_models(cuda)
    for c3, c2 in zip(convs3, convs2):
        c3.load_state_dict(c2.state_dict())
        for mod in c3.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.add_(0.05)
                mod.running_var.mul_(1.3)
    eng.load_bn_stats(convs3)
    after3 = _out(s.run(x[:batch]))
    want3 = _out(mk(convs3, fc2).session(batch, which="classical", routing="soft").run(x[:batch]))
    torch.cuda.synchronize()
    assert not _same(after3[0], after[0])
    assert all(_same(a, b) for a, b in zip(after3, want3))
    s.close()


# ================================================================================ 6. refusals
def test_refusals_are_value_errors(cuda, setup):
    eng, x = setup["eng"]["bf16"], setup["x"]
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import NoiseModel
    for batch in (0, 17, -1, 2.0):
        with pytest.raises(ValueError):
            eng.session(batch)
    with pytest.raises(ValueError):
        eng.session(4, which="classical", shots=100)
    with pytest.raises(ValueError):
        eng.session(4, which=None, shots=100)
    with pytest.raises(ValueError):
        eng.session(4, which="quantum", noise=NoiseModel(p1=0.01))      # (noise needs shots)
    with pytest.raises(ValueError):
        eng.session(4, which="nearest")
    with pytest.raises(ValueError):
        eng.session(4, routing="top2")
    with pytest.raises(ValueError):   # (no classical classifier loaded)
        HIPInference(setup["convs"], setup["fc"], 128, cuda, chunk=48).session(4, which="classical")
    # soft routing with a classifier of another class count
    torch.manual_seed(1)
    q4 = QSC_P128(8, 3, 4, False, False, 128).to(cuda).eval()
    e4 = HIPInference(setup["convs"], setup["fc"], 128, cuda, chunk=48, qsc=q4)
    with pytest.raises(ValueError):
        e4.session(4, which="quantum", routing="soft")
    # an FC shape the skinny kernels do not take
    e4.W_lp = e4.W_lp[:, :4096 - 256].contiguous()
    with pytest.raises(ValueError):
        e4.session(4, which=None)
    # run: wrong batch / shape, missing routing input
    s = eng.session(4, which=None)
    Y0 = s.Y.clone()
    for bad in (x[:5], x[:3], x[:4, :1], x[:4].reshape(4, 2, 8, 16)):
        with pytest.raises(ValueError):
            s.run(bad, expert=torch.zeros(4, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        s.run(x[:4])
    with pytest.raises(ValueError):
        s.run(x[:4], expert=torch.zeros(5, dtype=torch.int64, device=cuda))
    s2 = eng.session(4, which=None, routing="soft")
    with pytest.raises(ValueError):
        s2.run(x[:4])
    with pytest.raises(ValueError):
        s2.run(x[:4], weights=torch.zeros(4, 2, device=cuda))
    s3 = eng.session(4, which="classical")
    with pytest.raises(ValueError):
        s3.run(x[:4], expert=torch.zeros(4, dtype=torch.int64, device=cuda))
    torch.cuda.synchronize()
    assert _same(s.Y, Y0), "a refused run launched"
    for t in (s, s2, s3):
        t.close()
    with pytest.raises(ValueError):
        s.run(x[:4], expert=torch.zeros(4, dtype=torch.int64, device=cuda))


# ================================================================================ 7. row independence, end to end
@pytest.mark.parametrize("routing", ["hard", "soft"])
@pytest.mark.parametrize("dt", ["bf16", "fp8"])
def test_sample_0_is_the_same_at_batch_1_and_batch_16(cuda, setup, dt, routing):
    eng, x = setup["eng"][dt], setup["x"]
    s1 = eng.session(1, which="quantum", routing=routing)
    s16 = eng.session(16, which="quantum", routing=routing)
    a, b = _out(s1.run(x[:1])), _out(s16.run(x[:16]))
    torch.cuda.synchronize()
    assert _same(a[0][0], b[0][0]) and _same(a[2][0], b[2][0]) and int(a[1][0]) == int(b[1][0])
    assert s1.launches == s16.launches and len(s1.launches) == (10 if dt == "bf16" else 11) + (routing == "soft")
    s1.close()
    s16.close()
