"""csrc/hip/qsc_postmeas.hip (QuantumNAT post-measurement normalization / quantization fused into the QSC heads) and
its wiring, against ops/postmeas.py's fp64 composition.

The per-element bound (``oracle``) for z, dE and the running buffers, first order in u = 2^-24 (fp32 unit round-off):
a block sum is D = ceil(B / 1024) + 6 + 16 sequential roundings deep (a thread's rows, the wave butterfly, the 16
wave partials), so

  mu     : e_mu = (D + 1) u mean|E_j|
  v      : relative e_v = (D + 5) u + e_mu^2 / v        (the centred two-pass sum: first order in e_mu vanishes)
  rstd   : relative e_r = e_v / 2 + 3 u                 (add eps, sqrt, divide)
  z      : |z| (e_r + 2 u) + e_mu / sigma_j             <- 1 / sigma_min enters here; inputs have sigma_j >= 0.05
  run_*  : momentum times the above, plus 4 u of the blended terms
  dE     : the same calculus through y (K >= 2: the SAME level by construction, 6 u R of rounding in -R + D k), the
           logits ((n + 2) u), the softmax (__expf / __logf taken as (4 + 2 |x|) u relative / 3 u |log| + 2 u
           absolute), g, the two per-wire means ((D + 2) u, (D + 3) u) and rstd (g - mean g - z mean(g z)).

Quantized cases generate E so that every fp64 z is >= 1e-3 D from a rounding boundary and from +-qrange (asserted),
and then compare ALL elements.  Loss and weight-gradient tolerances are tests/test_qsc_gpu.py's."""
import ctypes
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.postmeas import post_measurement
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import NoiseModel

from test_postmeas_cpu import away_from_boundaries, make_inputs

pytestmark = pytest.mark.gpu

_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
F64 = torch.float64
U = 2.0 ** -24
MOM, EPS, R = 0.1, 1e-5, 2.0
WORST = {}   # kind -> worst error / bound ratio seen (printed by the tests)


def head_fn():
    return nat.fn(nat.hip_lib(), "qd_qsc_head_pm", [_p] * 10 + [_i] * 5 + [_p, _p, _f, _f, _i, _f, _f, _p, _p])


def infer_fn():
    return nat.fn(nat.hip_lib(), "qd_qsc_infer_head_pm", [_p] * 5 + [_i] * 5 + [_p, _p, _f, _i, _f, _p])


def oracle(E, wc, bc, lab, rm0, rv0, K, qw, training=True):
    """fp64 values of the head (closed form, checked against autograd through ops.postmeas) and the per-element fp32
    error bounds of the module docstring.  All tensors on the CPU."""
    E, wc, bc, rm0, rv0 = E.double(), wc.double(), bc.double(), rm0.double(), rv0.double()
    B, n = E.shape
    C = wc.shape[0]
    D = -(-B // 1024) + 6 + 16
    mu = E.mean(0)
    c = E - mu
    v = (c * c).mean(0)
    rstd = torch.rsqrt(v + EPS)
    z = c * rstd
    e_mu = (D + 1) * U * E.abs().mean(0)
    e_v = (D + 5) * U + e_mu ** 2 / v
    e_r = 0.5 * e_v + 3 * U
    b_z = z.abs() * (e_r + 2 * U) + e_mu * rstd
    if K >= 2:
        d = 2 * R / (K - 1)
        y = -R + d * torch.round((z.clamp(-R, R) + R) / d)
        b_y = torch.full_like(z, 6 * U * R)
        r = z - y
        mask = (z.abs() <= R).double()
    else:
        y, b_y, r, mask = z, b_z, torch.zeros_like(z), torch.ones_like(z)
    pw = qw / (B * n) if K >= 2 else 0.0
    awc = wc.abs()
    lg = y @ wc.T + bc
    b_lg = b_y @ awc.T + (n + 2) * U * (y.abs() @ awc.T + bc.abs())
    mx = lg.max(1, keepdim=True).values
    x = lg - mx
    se = torch.exp(x).sum(1, keepdim=True)
    lse = mx + torch.log(se)
    e_exp = lambda a: (4 + 2 * a.abs()) * U
    b_lse = (b_lg.max(1, keepdim=True).values + e_exp(x).max(1, keepdim=True).values + C * U
             + 3 * U * torch.log(se).abs() + 2 * U + U * (mx.abs() + lse.abs()))
    a = lg - lse
    p = torch.exp(a)
    b_p = p * (b_lg + b_lse + U * a.abs() + e_exp(a))
    oh = F.one_hot(lab, C).double()
    gl = (p - oh) / B
    b_gl = (b_p + 2 * U * (p - oh).abs()) / B
    dy = gl @ wc
    b_dy = b_gl @ awc + (C + 1) * U * (gl.abs() @ awc)
    g = mask * dy + 2 * pw * r
    b_g = mask * b_dy + 2 * pw * (b_z + b_y + 4 * U * r.abs()) + U * g.abs()
    mg = g.mean(0)
    b_mg = b_g.mean(0) + (D + 2) * U * g.abs().mean(0)
    mgz = (g * z).mean(0)
    b_mgz = (b_g * z.abs() + g.abs() * b_z).mean(0) + (D + 3) * U * (g * z).abs().mean(0)
    inner = g - mg - z * mgz
    b_in = b_g + b_mg + z.abs() * b_mgz + mgz.abs() * b_z + 4 * U * (g.abs() + mg.abs() + (z * mgz).abs())
    dE = rstd * inner
    b_dE = rstd * b_in + dE.abs() * (e_r + U)
    vun = v * B / (B - 1)
    rm = (1 - MOM) * rm0 + MOM * mu
    rv = (1 - MOM) * rv0 + MOM * vun
    b_rm = MOM * e_mu + 4 * U * (rm0.abs() + mu.abs())
    b_rv = MOM * vun * (e_v + 3 * U) + 4 * U * (rv0.abs() + vun)
    nll = (lse.squeeze(1) - (lg * oh).sum(1)).mean()
    loss = nll + pw * (r * r).sum()
    dwc = gl.T @ y
    dbc = gl.sum(0)
    # the closed form IS the oracle's autograd
    Ea, wa, ba = E.clone().requires_grad_(True), wc.clone().requires_grad_(True), bc.clone().requires_grad_(True)
    rma, rva = rm0.clone(), rv0.clone()
    ya, za, pen = post_measurement(Ea, rma, rva, training=True, stats="batch", momentum=MOM, eps=EPS, levels=K,
                                   qrange=R)
    la = F.nll_loss(F.log_softmax(ya @ wa.T + ba, 1), lab) + qw * pen / (B * n)
    la.backward()
    for got, want in ((z, za.detach()), (dE, Ea.grad), (dwc, wa.grad), (dbc, ba.grad), (rm, rma), (rv, rva),
                      (loss, la.detach())):
        assert (got - want).abs().max() <= 1e-10 * max(1.0, float(want.abs().max()))
    return dict(z=z, dE=dE, rm=rm, rv=rv, loss=loss, dwc=dwc, dbc=dbc, y=y,
                b_z=b_z, b_dE=b_dE, b_rm=b_rm, b_rv=b_rv)


def check_bound(kind, got, want, bound):
    err = (got.double().cpu() - want).abs()
    ratio = float((err / bound).max())
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    assert bool((err <= bound).all()), (kind, ratio, float(err.max()))


def head_inputs(B, n, C, K, seed, dev):
    E = make_inputs(B, n, K, R, seed, dtype=torch.float32)
    if K >= 2:
        assert bool(away_from_boundaries(E.double(), K, R, EPS).all())
    assert float(E.double().std(0, unbiased=False).min()) >= 0.05
    g = torch.Generator().manual_seed(seed + 1)
    wc = torch.randn(C, n, generator=g) * 0.5
    bc = torch.randn(C, generator=g) * 0.1
    lab = torch.randint(0, C, (B,), generator=g)
    rm0 = torch.randn(n, generator=g) * 0.1
    rv0 = 0.5 + torch.rand(n, generator=g)
    return E, wc, bc, lab, rm0, rv0


def launch_head(dev, E, wc, bc, lab, rm0, rv0, K, qw, accumulate, pre=None, skip=None, skip_add=0):
    B, n = E.shape
    C = wc.shape[0]
    t = dict(E=E.to(dev), wc=wc.to(dev), bc=bc.to(dev), lab=lab.to(dev), rm=rm0.clone().to(dev), rv=rv0.clone().to(dev),
             dE=torch.full((B, n), -7.0, device=dev), z=torch.full((B, n), -7.0, device=dev),
             dwc=(pre[0].clone().to(dev) if pre else torch.full((C, n), -7.0, device=dev)),
             dbc=(pre[1].clone().to(dev) if pre else torch.full((C,), -7.0, device=dev)),
             loss=torch.full((1,), -7.0, device=dev), lacc=torch.ones(1, device=dev))
    st = head_fn()(nat.ptr(t["E"]), nat.ptr(t["wc"]), nat.ptr(t["bc"]), nat.ptr(t["lab"]), nat.ptr(t["dE"]),
                   nat.ptr(t["dwc"]), nat.ptr(t["dbc"]), nat.ptr(t["loss"]), nat.ptr(t["lacc"]),
                   nat.ptr(skip) if skip is not None else None, skip_add, int(accumulate), B, n, C, nat.ptr(t["rm"]),
                   nat.ptr(t["rv"]), MOM, EPS, K, R, qw, nat.ptr(t["z"]), nat.stream_ptr(dev))
    assert st == 0, st
    torch.cuda.synchronize()
    return t


# (B, n, C): the smallest legal shape; one row past a wave; one row past the workgroup (second trip); the step's shape
# (three register-kept rows per thread); n > 8 (rows re-read from E) with 4 classes; the widest head; a fourth trip
# after the three kept rows (the tail loop that re-reads E; 9 x 512 samples reach it); three trips of re-read rows
HEAD_SHAPES = [(2, 2, 2), (65, 3, 3), (1025, 8, 3), (2304, 8, 3), (72, 12, 4), (18, 16, 2), (3100, 8, 3), (2100, 12, 3)]


@pytest.mark.parametrize("B,n,C", HEAD_SHAPES)
def test_head_pm_matches_fp64_composition(cuda, B, n, C):
    for K in (0, 2, 5, 6):
        E, wc, bc, lab, rm0, rv0 = head_inputs(B, n, C, K, 100 * n + K, cuda)
        for qw in (0.0, 0.1):
            ref = oracle(E, wc, bc, lab, rm0, rv0, K, qw)
            pre = (torch.randn(C, n), torch.randn(C))
            for accumulate in (0, 1):
                t = launch_head(cuda, E, wc, bc, lab, rm0, rv0, K, qw, accumulate, pre=pre)
                assert torch.allclose(t["loss"][0].double().cpu(), ref["loss"], rtol=1e-4, atol=1e-5), (K, qw)
                assert torch.allclose(t["lacc"][0].double().cpu(), 1.0 + ref["loss"], rtol=1e-4, atol=1e-5)
                for name, base in (("dwc", pre[0]), ("dbc", pre[1])):
                    got = t[name].double().cpu() - (base.double() if accumulate else 0.0)
                    err = (got - ref[name]).abs().max() / ref[name].abs().max().clamp_min(1e-12)
                    slack = 8 * U * float(base.abs().max()) / float(ref[name].abs().max().clamp_min(1e-12)) \
                        if accumulate else 0.0   # (the sum with the fp32 value already there rounds once more)
                    assert err < 2e-3 + slack, (name, K, qw, accumulate, float(err))
                check_bound("z", t["z"], ref["z"], ref["b_z"])
                check_bound("dE", t["dE"], ref["dE"], ref["b_dE"])
                check_bound("running_mean", t["rm"], ref["rm"], ref["b_rm"])
                check_bound("running_var", t["rv"], ref["rv"], ref["b_rv"])
                # bit-identical run to run
                t2 = launch_head(cuda, E, wc, bc, lab, rm0, rv0, K, qw, accumulate, pre=pre)
                for k in ("dE", "z", "dwc", "dbc", "loss", "rm", "rv"):
                    assert torch.equal(t[k], t2[k]), k
    print(f"head_pm ({B}, {n}, {C}): worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


def test_head_pm_refuses_bad_arguments(cuda):
    E, wc, bc, lab, rm0, rv0 = head_inputs(4, 3, 3, 0, 1, cuda)
    buf = {k: v.to(cuda) for k, v in dict(E=E, wc=wc, bc=bc, lab=lab, rm=rm0, rv=rv0).items()}
    out = torch.full((64,), -7.0, device=cuda)
    f = head_fn()

    def call(B=4, n=3, C=3, K=0, qr=R):
        return f(nat.ptr(buf["E"]), nat.ptr(buf["wc"]), nat.ptr(buf["bc"]), nat.ptr(buf["lab"]), nat.ptr(out),
                 nat.ptr(out[16:]), nat.ptr(out[32:]), nat.ptr(out[40:]), None, None, 0, 0, B, n, C, nat.ptr(buf["rm"]),
                 nat.ptr(buf["rv"]), MOM, EPS, K, qr, 0.0, None, nat.stream_ptr(cuda))

    assert call(K=1) == 1 and call(B=1) == 1 and call(qr=0.0) == 1 and call(qr=-1.0) == 1
    assert call(n=17) == 1 and call(C=5) == 1 and call(K=-1) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and torch.equal(buf["rm"].cpu(), rm0)   # nothing was launched
    fi = infer_fn()
    ci = lambda **k: fi(nat.ptr(buf["E"]), nat.ptr(buf["wc"]), nat.ptr(buf["bc"]), nat.ptr(out), None, 4, 3, 3,
                        k.get("valid", 4), k.get("mode", 0), nat.ptr(buf["rm"]), nat.ptr(buf["rv"]), EPS,
                        k.get("K", 0), k.get("qr", R), nat.stream_ptr(cuda))
    assert ci(valid=0) == 1 and ci(valid=5) == 1 and ci(mode=2) == 1 and ci(K=1) == 1 and ci(qr=0.0) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_head_pm_nonfinite_loss_leaves_running_statistics(cuda):
    E, wc, bc, lab, rm0, rv0 = head_inputs(300, 4, 3, 5, 7, cuda)
    skip = torch.zeros(1, device=cuda)
    t = launch_head(cuda, E, wc, bc, lab, rm0, rv0, 5, 0.1, 0, skip=skip)
    assert float(skip) == 0.0 and not torch.equal(t["rm"].cpu(), rm0) and not torch.equal(t["rv"].cpu(), rv0)
    bad = E.clone()
    bad[137, 2] = float("nan")
    skip.fill_(5.0)
    t = launch_head(cuda, bad, wc, bc, lab, rm0, rv0, 5, 0.1, 0, skip=skip)
    assert float(skip) == 1.0 and not math.isfinite(float(t["loss"]))
    assert torch.equal(t["rm"].cpu(), rm0) and torch.equal(t["rv"].cpu(), rv0)      # bit-identical to before
    skip.fill_(2.0)
    t = launch_head(cuda, bad, wc, bc, lab, rm0, rv0, 5, 0.1, 0, skip=skip, skip_add=1)
    assert float(skip) == 3.0
    assert torch.equal(t["rm"].cpu(), rm0) and torch.equal(t["rv"].cpu(), rv0)
    t = launch_head(cuda, E, wc, bc, lab, rm0, rv0, 5, 0.1, 0, skip=skip, skip_add=1)
    assert float(skip) == 3.0 and not torch.equal(t["rm"].cpu(), rm0)


def test_head_pm_graph_replays_move_the_buffers_like_eager_launches(cuda):
    B, n, C, K = 300, 8, 3, 5
    E, wc, bc, lab, rm0, rv0 = head_inputs(B, n, C, K, 9, cuda)
    dv = {k: v.to(cuda) for k, v in dict(E=E, wc=wc, bc=bc, lab=lab).items()}
    outs = []
    for graphed in (False, True):
        rm, rv = rm0.clone().to(cuda), rv0.clone().to(cuda)
        dE, dwc, dbc, loss = (torch.zeros(B, n, device=cuda), torch.zeros(C, n, device=cuda),
                              torch.zeros(C, device=cuda), torch.zeros(1, device=cuda))

        def launch():
            nat.check(head_fn()(nat.ptr(dv["E"]), nat.ptr(dv["wc"]), nat.ptr(dv["bc"]), nat.ptr(dv["lab"]), nat.ptr(dE),
                                nat.ptr(dwc), nat.ptr(dbc), nat.ptr(loss), None, None, 0, 0, B, n, C, nat.ptr(rm),
                                nat.ptr(rv), MOM, EPS, K, R, 0.1, None, nat.stream_ptr(cuda)), "qsc_head_pm")

        if graphed:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(graph, stream=s):
                    launch()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)   # capture launched nothing
            for _ in range(3):
                graph.replay()
        else:
            for _ in range(3):
                launch()
        torch.cuda.synchronize()
        outs.append((rm.clone(), rv.clone(), dE.clone(), loss.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0].cpu(), rm0)


@pytest.mark.parametrize("pattern", [0xFFFFFFFF, 0x7F7F7F7F])
def test_head_pm_lds_poison(cuda, pattern):
    """Every LDS word the kernels read was written by the same launch: poisoned runs are bit-identical."""
    E, wc, bc, lab, rm0, rv0 = head_inputs(2304, 8, 3, 5, 21, cuda)
    clean = launch_head(cuda, E, wc, bc, lab, rm0, rv0, 5, 0.1, 0)
    try:
        nat.set_lds_poison(pattern)
        poisoned = launch_head(cuda, E, wc, bc, lab, rm0, rv0, 5, 0.1, 0)
    finally:
        nat.set_lds_poison(None)
    for k in ("dE", "z", "dwc", "dbc", "loss", "rm", "rv"):
        assert torch.equal(clean[k], poisoned[k]), k
    assert bool(torch.isfinite(clean["dE"]).all())


@pytest.mark.parametrize("mode", ["batch", "running"])
@pytest.mark.parametrize("B,valid", [(2, 2), (300, 257), (4096, 4095)])
def test_infer_head_pm(cuda, B, valid, mode):
    n, C = 8, 3
    for K in (0, 5):
        g = torch.Generator().manual_seed(B + K)
        rm0 = torch.randn(n, generator=g) * 0.05
        rv0 = 0.05 + 0.1 * torch.rand(n, generator=g)
        for k in range(64):   # valid rows whose z (under the mode's statistics) sit away from the boundaries
            Ev = make_inputs(valid, n, K if mode == "batch" else 0, R, 50 * B + K + 1000 * k, dtype=torch.float32)
            if K < 2 or mode == "batch":
                break
            zr = (Ev.double() - rm0.double()) * torch.rsqrt(rv0.double() + EPS)
            d = 2 * R / (K - 1)
            uu = (zr.clamp(-R, R) + R) / d
            bad = ((uu - uu.floor() - 0.5).abs() < 1e-3) | (((zr.abs() - R).abs() / d) < 1e-3)
            Ev = Ev + bad * 0.004
            zr = (Ev.double() - rm0.double()) * torch.rsqrt(rv0.double() + EPS)
            uu = (zr.clamp(-R, R) + R) / d
            if not bool((((uu - uu.floor() - 0.5).abs() < 1e-3) | (((zr.abs() - R).abs() / d) < 1e-3)).any()):
                break
        else:
            raise AssertionError("no input away from the boundaries")
        E = torch.cat([Ev, Ev[-1:].expand(B - valid, n)]).contiguous()   # the padding repeats a sample
        y, z, _ = post_measurement(Ev.double(), rm0.double(), rv0.double(), training=False, stats=mode, eps=EPS, levels=K,
                                   qrange=R)
        if K >= 2 and mode == "batch":
            assert bool(away_from_boundaries(Ev.double(), K, R, EPS).all())
        for _ in range(64):   # a head under which no valid row has its two largest logits within 1e-4: pred is exact
            wc = torch.randn(C, n, generator=g)
            bc = torch.randn(C, generator=g) * 0.1
            lg = y @ wc.double().T + bc.double()
            top = lg.topk(2, 1).values
            if float((top[:, 0] - top[:, 1]).min()) > 1e-4:
                break
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
        ref = torch.log_softmax(lg, 1)
        logp = torch.full((B, C), -7.0, device=cuda)
        pred = torch.full((B,), -7, dtype=torch.int64, device=cuda)
        dv = [t.to(cuda) for t in (E, wc, bc, rm0, rv0)]
        nat.check(infer_fn()(nat.ptr(dv[0]), nat.ptr(dv[1]), nat.ptr(dv[2]), nat.ptr(logp), nat.ptr(pred), B, n, C,
                             valid, int(mode == "running"), nat.ptr(dv[3]), nat.ptr(dv[4]), EPS, K, R,
                             nat.stream_ptr(cuda)), "qsc_infer_head_pm")
        torch.cuda.synchronize()
        err = float((logp[:valid].double().cpu() - ref).abs().max())
        assert err <= 1e-5, (K, err)
        assert torch.equal(pred[:valid].cpu(), ref.argmax(1))
        assert bool(torch.isfinite(logp).all()) and bool(((pred >= 0) & (pred < C)).all())   # every row got an output
        assert torch.equal(dv[3].cpu(), rm0) and torch.equal(dv[4].cpu(), rv0)


# ---------------------------------------------------------------------------------------------- the fused step
def _pair(dev, pilot_num, n, B, impl="mfma", post=None, L=3, **kw):
    """(model with post-processing, its space and step, the same model without, its step, x, labels)."""
    post = post if post is not None else dict(post_norm=True)
    H, W = (16, 8) if pilot_num == 128 else (16, 16)
    torch.manual_seed(0)
    a = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False, pilot_num=pilot_num,
                 **post).to(dev).train()
    p = QSC_P128(n_qubits=n, n_layers=L, use_quantumnat=False, use_gradient_pruning=False,
                 pilot_num=pilot_num).to(dev).train()
    p.load_state_dict({k: v for k, v in a.state_dict().items() if "postmeas" not in k})
    sa, sp = FlatParamSpace(list(a.named_parameters()), dev), FlatParamSpace(list(p.named_parameters()), dev)
    return a, sa, QSCStepHIP(a, sa, B, impl=impl, **kw), p, sp, QSCStepHIP(p, sp, B, impl=impl, **kw), H, W


@pytest.mark.parametrize("impl", ["mfma", "ref"])
@pytest.mark.parametrize("pilot_num,n,B", [(128, 8, 2304), (128, 4, 300), (256, 12, 72)])
def test_step_matches_autograd_through_the_module(cuda, pilot_num, n, B, impl):
    """Normalization alone (no quantization decision is compared between the kernel's fp32 E and torch's)."""
    a, sa, step, p, sp, plain, H, W = _pair(cuda, pilot_num, n, B, impl)
    b = QSC_P128(n_qubits=n, use_quantumnat=False, use_gradient_pruning=False, pilot_num=pilot_num,
                 post_norm=True).to(cuda).train()
    b.load_state_dict(a.state_dict())
    x = torch.randn(B, 2, H, W, device=cuda)
    y = torch.randint(0, 3, (B,), device=cuda)
    sa.zero_grad()
    sp.zero_grad()
    loss = step(x, y)
    plain(x, y)
    ref = F.nll_loss(b(x), y) + b.postmeas.penalty
    ref.backward()
    torch.cuda.synchronize()
    assert torch.equal(step.E, plain.E)            # the measurement is untouched
    assert torch.allclose(loss[0], ref, rtol=1e-4, atol=1e-5), (loss, ref)
    for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert na == nb
        err = (pa.grad - pb.grad).abs().max() / pb.grad.abs().max().clamp_min(1e-12)
        assert err < 2e-3, (na, float(err))
    for k in ("running_mean", "running_var"):
        ta, tb = getattr(a.postmeas, k), getattr(b.postmeas, k)
        assert float((ta - tb).abs().max()) <= 1e-5 and not torch.equal(ta, torch.zeros_like(ta))
    # dE -- what the adjoint backward consumed -- is the composition's backward on the step's own E
    cls = a.classifier
    ref = oracle(step.E.cpu(), cls.weight.detach().cpu(), cls.bias.detach().cpu(), y.cpu(), torch.zeros(n),
                 torch.ones(n), 0, 0.0)
    check_bound("step dE", step.dE, ref["dE"], ref["b_dE"])
    check_bound("step running_var", a.postmeas.running_var, ref["rv"], ref["b_rv"])


@pytest.mark.parametrize("mode", ["shots", "noisy_adjoint"])
def test_measured_step_with_quantization(cuda, mode):
    """shots = 256 plain / noisy_adjoint, n = 4, B = 64, 5 levels: E is the plain step's bit for bit, and the head's
    outputs (dE -- what the mode's backward kernel consumes --, z's running statistics, the head gradients) are the
    fp64 composition's on that E.  The x draw is the first of 16 whose measured E clears the boundary margin."""
    n, B, K, qw = 4, 64, 5, 0.1
    kw = dict(shots=256) if mode == "shots" else dict(
        shots=256, noise=NoiseModel(1e-3, 1e-2, 0.02, 0.02), trajectories=4, diff_method="noisy_adjoint")
    post = dict(post_norm=True, post_quant_levels=K, post_quant_weight=qw)
    for seed in range(16):
        a, sa, step, p, sp, plain, H, W = _pair(cuda, 128, n, B, post=post, L=2, shot_seed=3, **kw)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, 2, H, W, generator=g).to(cuda)
        y = torch.randint(0, 3, (B,), generator=g).to(cuda)
        sa.zero_grad()
        sp.zero_grad()
        loss = step(x, y)
        plain(x, y)
        torch.cuda.synchronize()
        assert step.measured and torch.equal(step.E, plain.E) and int(step.shot_ctr) == 1
        E = step.E.cpu()
        if bool(away_from_boundaries(E.double(), K, R, EPS).all()):
            break
    else:
        raise AssertionError("no draw away from the boundaries")
    cls = a.classifier
    ref = oracle(E, cls.weight.detach().cpu(), cls.bias.detach().cpu(), y.cpu(), torch.zeros(n), torch.ones(n), K, qw)
    assert torch.allclose(loss[0].double().cpu(), ref["loss"], rtol=1e-4, atol=1e-5)
    check_bound("step dE", step.dE, ref["dE"], ref["b_dE"])
    check_bound("step running_mean", a.postmeas.running_mean, ref["rm"], ref["b_rm"])
    check_bound("step running_var", a.postmeas.running_var, ref["rv"], ref["b_rv"])
    err = (cls.weight.grad.double().cpu() - ref["dwc"]).abs().max() / ref["dwc"].abs().max()
    assert err < 2e-3, float(err)
    assert not torch.equal(step.dE, plain.dE) and float(a.qlayer.weights.grad.abs().max()) > 0
    assert bool(torch.isfinite(sa.grad).all())


def test_classifier_step_infer_chunks(cuda):
    """ClassifierStep._infer_hip with N no multiple of the static batch: every chunk is normalized with the statistics
    of its own valid rows (the padding stays out), quantized and classified -- the fp64 composition chunk by chunk on
    the E the kernels measured for that chunk (recorded after every QSCStepHIP.infer).  E comes from the circuit: per
    statistics mode, x is the first of 32 draws for which every valid row of every chunk clears the 1e-3 D margin
    (asserted); then all N rows are compared."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import ClassifierStep
    n, Bs, K = 4, 32, 5
    N = 2 * Bs + 5
    torch.manual_seed(3)
    m = QSC_P128(n_qubits=n, use_quantumnat=True, use_gradient_pruning=False, post_norm=True,
                 post_quant_levels=K).to(cuda)
    m.postmeas.running_mean.copy_(torch.tensor([0.05, -0.1, 0.0, 0.1]))
    m.postmeas.running_var.copy_(torch.tensor([0.05, 0.1, 0.08, 0.06]))
    space = FlatParamSpace(list(m.named_parameters()), cuda)
    cs = ClassifierStep(m, 1, space=space, batch_total=Bs)
    m.eval()
    rec, infer = [], cs.hip.infer

    def spy(*a, **k):
        infer(*a, **k)
        torch.cuda.synchronize()
        rec.append((cs.hip.E.clone(), k.get("valid")))

    cs.hip.infer = spy
    d = 2 * R / (K - 1)
    wc, bc = m.classifier.weight.detach().double(), m.classifier.bias.detach().double()
    for stats in ("running", "batch"):
        m.postmeas.stats = stats
        for seed in range(32):
            x = torch.randn(N, 2, 16, 8, generator=torch.Generator().manual_seed(seed)).to(cuda)
            rec.clear()
            got = cs.forward(x)
            torch.cuda.synchronize()
            assert [v for _, v in rec] == [Bs, Bs, 5] and got.shape == (N, 3)
            ref, clear = [], True
            for E, valid in rec:
                yq, z, _ = post_measurement(E[:valid].double(), m.postmeas.running_mean.double(),
                                            m.postmeas.running_var.double(), training=False, stats=stats, levels=K)
                uu = (z.clamp(-R, R) + R) / d
                clear &= not bool((((uu - uu.floor() - 0.5).abs() < 1e-3) | (((z.abs() - R).abs() / d) < 1e-3)).any())
                ref.append(torch.log_softmax(yq @ wc.T + bc, 1))
            if clear:
                break
        assert clear, "no draw away from the boundaries"
        err = float((got.double() - torch.cat(ref)).abs().max())   # all N rows
        assert err <= 1e-5, (stats, err)
    # batch mode: a prediction depends on the chunk it is in
    assert not torch.equal(cs.forward(x[Bs:Bs + 5]), got[Bs:Bs + 5])


def test_runner_fused_graphed_with_postmeas(cuda, tmp_path, monkeypatch):
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train import runner as rn
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train import checkpoint as ck
    import glob
    seen = []
    real = rn._capture_preserving

    def spy(graphed, state, static_idx, idx):
        post = state[-2:]   # the two running-statistics buffers are the last entries of the snapshot
        assert all(t.shape == (4,) and t.dtype == torch.float32 for t in post)
        before = [t.clone() for t in post]
        real(graphed, state, static_idx, idx)
        seen.append((before, [t.clone() for t in post]))

    monkeypatch.setattr(rn, "_capture_preserving", spy)

    def runner(**kw):
        return rn.Y2HRunner(n_epochs=2, data_len=60, batch_size_DML=16, device="cuda", workspace=str(tmp_path / "w"),
                            data_dir=str(tmp_path / "data"), print_freq=1000, n_qubits=4, n_layers=2,
                            use_quantumnat=True, seed=0, qsc_diff_method="noisy_adjoint", qsc_shots=64,
                            qsc_noise_p1=1e-3, qsc_noise_p2=1e-2, qsc_readout01=0.02, qsc_readout10=0.02,
                            qsc_trajectories=4, qsc_step="fused", qsc_post_norm=True, qsc_post_quant_levels=5,
                            qsc_post_quant_weight=0.1, **kw)

    r = runner()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = r.train_QSC_P128()
    assert len(seen) == 1
    before, after = seen[0]
    assert torch.equal(before[0], torch.zeros(4, device=cuda)) and torch.equal(before[1], torch.ones(4, device=cuda))
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])   # warm-up replays moved nothing
    assert all(math.isfinite(v) for v in r.train_QSC_losses) and len(r.train_QSC_losses) == 2
    rm, rv = m.postmeas.running_mean.clone(), m.postmeas.running_var.clone()
    assert not torch.equal(rm, before[0]) and bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rv).all())
    files = glob.glob(str(tmp_path / "w" / "**" / "QSC_*_resume.pth"), recursive=True)
    st = ck.load_resume(files[0])
    assert torch.equal(st["postmeas"][0], rm.cpu()) and torch.equal(st["postmeas"][1], rv.cpu())
    # a resumed run starts from those buffers: nothing left to train, so it ends with them
    r2 = runner(resume=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2 = r2.train_QSC_P128()
    assert torch.equal(m2.postmeas.running_mean, rm) and torch.equal(m2.postmeas.running_var, rv)
