"""The conv / BN / ReLU oracle (tests/conv_oracle.py) checked against itself and against torch autograd, no GPU:
the reference the exact GPU tests compare the kernels with is pinned to the operation, not to the kernels."""
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co

D = torch.float64
# (U, B) of tests/test_conv_exact_gpu.py
SHAPES = [(1, 1), (2, 5), (3, 13), (8, 2), (2, 9)]


def test_round_bf16_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 257.0, 259.0, -3.0, 0.0, 1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=D)
    # 1 + 2^-8 is a tie -> even (1.0); 1 + 3 * 2^-8 is a tie -> even (1 + 2^-6); 257 -> 256 (tie, even); 259 -> 260
    ref = torch.tensor([1.0, 1.0, 1.015625, 256.0, 260.0, -3.0, 0.0, 1.0078125], dtype=D)
    assert torch.equal(co.round_bf16(x), ref)
    # the last value rounds UP in one rounding; through fp32 first it would become the tie 1 + 2^-8 and round down
    assert float(x[-1].to(torch.float32).to(torch.bfloat16)) == 1.0
    y = torch.randn(4096, dtype=D)
    assert torch.equal(co.round_bf16(y.to(torch.float32).to(D)), y.to(torch.float32).to(torch.bfloat16).to(D))


@pytest.mark.parametrize("W", [8, 16])
@pytest.mark.parametrize("U,B", [(2, 5), (3, 2)])
@pytest.mark.parametrize("cin", [2, 32])
def test_oracle_backward_equals_autograd(U, B, W, cin):
    """conv2d -> batch_norm(training, per group of B samples) -> relu in float64 autograd, against the oracle's dx, dW,
    dgamma = sum g xhat, dbeta = sum g with records built from true batch statistics: to 1e-10."""
    torch.manual_seed(3)
    E, EC, eps = co.E, co.E * co.CO, 1e-5
    N = U * B
    h = torch.randn(N, E * cin, co.H, W, dtype=D, requires_grad=True)
    w = (0.2 * torch.randn(EC, cin, 3, 3, dtype=D)).requires_grad_(True)
    gamma = (torch.randn(EC, dtype=D).sign() * (0.5 + torch.rand(EC, dtype=D))).requires_grad_(True)   # both signs
    beta = (0.3 * torch.randn(EC, dtype=D)).requires_grad_(True)
    dh = torch.randn(N, EC, co.H, W, dtype=D)
    z = F.conv2d(h, w, padding=1, groups=E)
    out = torch.cat([F.relu(F.batch_norm(z[u * B:(u + 1) * B], None, None, gamma, beta, True, 0.0, eps))
                     for u in range(U)])
    dx_a, dw_a, dg_a, db_a = torch.autograd.grad(out, (h, w, gamma, beta), dh)

    zd = z.detach()
    rec, sg, sgx = co.bn_true_records(zd, dh, gamma.detach(), beta.detach(), U, eps)
    # the forward half of the records reproduces the module's output
    assert torch.allclose(torch.relu(co.per_n(rec["a"], B) * zd + co.per_n(rec["b"], B)), out.detach(), atol=1e-10, rtol=0)
    _, _, dz = co.bn_backward(dh, zd, rec, B, D)
    dx, dw = co.conv_grads(h.detach(), w.detach(), dz)
    for name, got, ref in (("dx", dx, dx_a), ("dW", dw, dw_a), ("dgamma", sgx.sum(0), dg_a), ("dbeta", sg.sum(0), db_a)):
        err = float((got - ref).abs().max())
        assert err < 1e-10, (name, err)


@pytest.mark.parametrize("W", [8, 16])
@pytest.mark.parametrize("U,B", SHAPES)
@pytest.mark.parametrize("seed", [0])   # (the seed test_conv_exact_gpu.py uses)
def test_lattice_is_exact(U, B, W, seed):
    """Every intermediate of the lattice data is representable where the kernels hold it (bf16 tiles and outputs,
    fp32 sums in any order, e4m3 operands), so a mismatch on the GPU is the kernel's."""
    c = co.case("lattice", U, B, W, seed)
    c.check_exact(f8=True)
    # and the data is not degenerate: gates of both kinds, negative slopes, non-trivial outputs
    b = c.bwd(3, True)
    assert 0.2 < float((b["g"] != 0).double().mean()) and float((b["dz"] != 0).double().mean()) > 0.5
    assert bool((c.prev["a"] < 0).any()) and bool((c.cur["a"] < 0).any())
    assert float(c.fwd(3)["z"].abs().max()) >= 8 and float(b["dx"].abs().max()) >= 8
    assert float((c.fwd(2)["h"] > 0).double().mean()) > 0.2


@pytest.mark.parametrize("W", [8, 16])
def test_impulse_is_exact_and_names_taps(W):
    c = co.impulse(1, 1, W)
    c.check_exact(f8=True)
    z = c.fwd(3)["z"][0, :co.CO]
    # output channel t holds tap t alone: the corner pixel (0, 0) (value 1) moved by (1 - kh, 1 - kw)
    for t in range(9):
        r, col = 1 - t // 3, 1 - t % 3
        if r >= 0 and col >= 0:
            assert float(z[t, r, col]) == 1.0, (t, z[t, :3, :3])
    assert float(z[9:].abs().max()) == 0.0


def test_real_case_operands_are_representable():
    c = co.case("real", 2, 5, 8, 0)
    for t in (c.z_prev, c.z, c.dh16, *c.wq):
        assert co.is_bf16(t)
    for rec in (c.prev, c.cur):
        for k in co.REC:
            assert co.is_f32(rec[k])
    assert co.is_f32(c.x1) and co.is_f32(c.dh32) and not co.is_bf16(c.dh32)
    assert bool((c.prev["a"] < 0).any()) and bool((c.prev["a"] > 0).any())
    # no h of the real cases sits where fp32 and float64 evaluation could round apart (the generator moved those),
    # and the fp32 evaluations -- fused or not -- do give the reference's h
    for U, B, W in ((2, 5, 8), (3, 13, 8), (2, 5, 16), (3, 13, 16), (2, 9, 8)):
        c = co.case("real", U, B, W, 0)
        assert not bool((co.h_flip_room(c.z_prev, c.prev["a"], c.prev["b"], B) > 0).any())
        a, b = co.per_n(c.prev["a"], B), co.per_n(c.prev["b"], B)
        f = torch.float32
        fused = torch.relu((a * c.z_prev + b).to(f)).to(torch.bfloat16).to(D)
        plain = torch.relu(a.to(f) * c.z_prev.to(f) + b.to(f)).to(torch.bfloat16).to(D)
        assert torch.equal(fused, c.h_in(2)) and torch.equal(plain, c.h_in(2))


def test_h_flip_room_finds_the_boundaries():
    one = torch.ones(1, 1, dtype=D)
    z = torch.tensor([1.0, 1.0 + 2.0 ** -8, 3.0, 0.0], dtype=D).view(1, 4, 1, 1)
    # y = z + b: b = 2^-8 puts z = 1 on the midpoint of 1 and 1 + 2^-7; b = 0 leaves bf16 values (no room) ...
    room = co.h_flip_room(z, one.expand(1, 4), (one * 2.0 ** -8).expand(1, 4), 1).flatten()
    assert float(room[0]) == 2.0 ** -7 and float(room[2]) == 0.0
    room = co.h_flip_room(z, one.expand(1, 4), (one * 0.0).expand(1, 4), 1).flatten()
    assert float(room[0]) == 0.0 and float(room[1]) == 2.0 ** -7 and float(room[2]) == 0.0   # ... z[1] is a midpoint


def test_bounds_catch_a_dropped_tap():
    """A simulated kernel (fp32 staging, bf16 h, fp32 conv, bf16 z) stays inside the forward bound; the same with
    one tap's contribution dropped in one output column does not."""
    c = co.case("real", 2, 5, 8, 0)
    f = c.fwd(3)
    f32 = torch.float32
    a, b = co.per_n(c.prev["a"], c.B).to(f32), co.per_n(c.prev["b"], c.B).to(f32)
    h = torch.relu(a * c.z_prev.to(f32) + b).to(torch.bfloat16).to(f32)
    w = c.wq[2].to(f32)
    z = F.conv2d(h, w, padding=1, groups=co.E).to(torch.bfloat16).to(D)
    ok = co.worst_ratio((z - f["z"]).abs(), co.fwd_bound(f["z"], f["S"]))
    assert ok <= 1.0, ok
    w2 = w.clone()
    w2[:, :, 1, 2] = 0
    zb = z.clone()
    zb[..., 3] = F.conv2d(h, w2, padding=1, groups=co.E).to(torch.bfloat16).to(D)[..., 3]
    bad = co.worst_ratio((zb - f["z"]).abs(), co.fwd_bound(f["z"], f["S"]))
    assert bad > 1.0, bad
    msg = co.mismatch("z", zb, z)
    assert msg is not None and "border" in msg and "interior" in msg and co.mismatch("z", z, z) is None
