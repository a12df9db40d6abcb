"""The FC GEMM oracle (tests/gemm_oracle.py) checked against itself, no GPU: the e4m3 rounding against torch's casts,
the lattice conditions, an fp32 emulation of every kernel output summed in shuffled orders and with K split in two
(bit-identical to the float64 reference on the lattice, inside the derived bounds on real data), and a list of
kernel defects applied to the emulated output -- each must be rejected by the check named for it, which is what
gives tests/test_gemm_exact_gpu.py its teeth."""
import pytest
import torch

import gemm_oracle as go

D, F32, BF = torch.float64, torch.float32, torch.bfloat16
I, J, K = 64, 64, 256       # emulated GEMM: 2 x 2 "tiles" of 32 x 32, 4 K steps of 64
T = 32


# ------------------------------------------------------------------------------------------ e4m3
def test_round_e4m3_matches_torch_casts():
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(F32).to(D)
    fin = codes[~torch.isnan(codes)]
    assert fin.numel() == 254 and float(fin.abs().max()) == 448.0 and float(fin[fin > 0].min()) == 2.0 ** -9
    assert torch.equal(go.round_e4m3(fin), fin)
    v = torch.sort(torch.unique(fin)).values
    mid = (v[:-1] + v[1:]) / 2                                       # every midpoint inside the finite range
    near = torch.cat([mid, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20)])
    x = torch.cat([near, (torch.rand(20000, dtype=D) * 2 - 1) * 448, torch.randn(20000, dtype=D) * 0.02])
    x = x.to(F32).to(D)                                              # (the cast under comparison starts from fp32)
    want = x.to(F32).to(torch.float8_e4m3fn).to(F32).to(D)
    assert torch.equal(go.round_e4m3(x), want)
    # ties go to the even code; the clamp comes first (no NaN above 448)
    assert torch.equal(go.round_e4m3(torch.tensor([17.0, 19.0, 1000.0, -1e9, 2.0 ** -10, 3 * 2.0 ** -10], dtype=D)),
                       torch.tensor([16.0, 20.0, 448.0, -448.0, 0.0, 2.0 ** -8], dtype=D))


# ------------------------------------------------------------------------------------------ emulated kernels
def emu_acc(g: go.Gemm, order: int, split: bool, P=None, Q=None) -> torch.Tensor:
    """The fp32 accumulator of P8 Q8^T: K permuted by ``order`` and, with ``split``, summed as two halves (KS = 2)."""
    P = (g.P8 if P is None else P).to(F32)
    Q = (g.Q8 if Q is None else Q).to(F32)
    perm = torch.randperm(g.K, generator=torch.Generator().manual_seed(order))
    P, Q = P[:, perm], Q[:, perm]
    if split:
        h = g.K // 2
        return P[:, :h] @ Q[:, :h].t() + P[:, h:] @ Q[:, h:].t()
    return P @ Q.t()


def emu_out(g: go.Gemm, acc: torch.Tensor, f32: bool, bias=None, trunc: bool = False) -> torch.Tensor:
    """The epilogue: accumulator x (sP sQ) (+ bias) in fp32, stored as fp32 or rounded once to bf16."""
    dq = torch.tensor(g.sP, dtype=F32) * torch.tensor(g.sQ, dtype=F32)
    v = acc * dq
    bias = g.bias if bias is None else bias
    if bias is not None:
        v = v + bias.to(F32)
    if f32:
        return v.to(D)
    return go.trunc_bf16(v.to(D)) if trunc else v.to(BF).to(D)


ORDERS = [(0, False), (1, False), (2, True), (3, True)]
CASES = [("bf16", True, False), ("bf16", False, True), ("bf16", False, False), ("e4m3", True, False),
         ("e4m3", False, True)]   # (format, bias, fp32 out): forward, wgrad, dgrad, e4m3 forward, e4m3 NT


@pytest.mark.parametrize("fmt,bias,f32", CASES)
def test_lattice_conditions_and_emulation_is_bit_exact(fmt, bias, f32):
    g = go.gemm("lattice", fmt, I, J, K, 0, bias)
    g.check_exact()
    assert f32 or g.n_ties > 0, "no bf16 tie among the sums: rounding modes are not distinguished"
    assert int((go.round_bf16(g.exact) != g.exact).sum()) > 0
    ref = g.out_f32() if f32 else g.out_bf16()
    for order, split in ORDERS:
        assert go.mismatch(f"{fmt} order {order}", emu_out(g, emu_acc(g, order, split), f32), ref) is None


@pytest.mark.parametrize("variant", ["scaled", "cancel"])
@pytest.mark.parametrize("fmt,bias,f32", CASES)
def test_real_emulation_is_inside_the_bounds(fmt, bias, f32, variant):
    g = go.gemm("real", fmt, I, J, K, 0, bias, variant)
    ref = g.out_f32()
    if variant == "cancel":
        assert float(g.exact.abs().median()) < 0.2 * float(g.S.median())
    for order, split in ORDERS:
        r = go.worst_ratio((emu_out(g, emu_acc(g, order, split), f32) - ref).abs(), g.bound(f32))
        assert r <= 1.0, (fmt, variant, order, r)


def test_routed_reference():
    A = torch.arange(24, dtype=D).reshape(12, 2)
    ex = torch.tensor([2, 0, 1, 1])
    assert torch.equal(go.route(A, ex, 3), A[[2, 3, 7, 10]])


# ------------------------------------------------------------------------------------------ BN partials
U, B, HW, BM = 2, 8, 8, 16      # M = 48, three 16-row tiles; the middle one straddles the groups at row 24


def bn_case(mode):
    M = 3 * U * B
    g = go.gemm(mode, "bf16", M, go.CPE * HW, 64, 1)
    return g, go.bn_z(mode, M, HW), go.bn_records(mode, U)


def emu_bn(dA, z, rec, order=0, gate_ge=False, charge_lo=False):
    """fp32 emulation of the BN reduction epilogue: part (U, M / BM, 2, 96), NaN where no row is shared."""
    M = dA.shape[0]
    part = torch.full((U, M // BM, 2, go.EC), float("nan"), dtype=D)
    gen = torch.Generator().manual_seed(order)
    f = lambda t: t.to(F32)
    for t in range(M // BM):
        u_lo = t * BM // (3 * B)
        for row in torch.randperm(BM, generator=gen).tolist():
            r = t * BM + row
            u_true, e = r // (3 * B), r % 3
            u = u_lo if charge_lo else u_true
            ch = slice(e * go.CPE, (e + 1) * go.CPE)
            rc = {k: f(rec[k][u_true, ch])[:, None] for k in ("mean", "inv", "a", "b")}
            zz, dd = f(z[r]).reshape(go.CPE, HW), f(dA[r]).reshape(go.CPE, HW)
            v = rc["a"] * zz + rc["b"]
            g = torch.where((v >= 0) if gate_ge else (v > 0), dd, torch.zeros((), dtype=F32))
            xh = (zz - rc["mean"]) * rc["inv"]
            perm = torch.randperm(HW, generator=gen)
            s1, s2 = g[:, perm].sum(1), (g * xh)[:, perm].sum(1)
            for k, s in ((0, s1), (1, s2)):
                cur = part[u, t, k, ch]
                part[u, t, k, ch] = (torch.where(torch.isnan(cur), torch.zeros((), dtype=D), cur).to(F32) + s).to(D)
    return part


def bn_verdict(mode, part, dA, z, rec):
    """(rows written where they must be, sums equal / inside the bound)."""
    refs = go.bn_partials(dA, z, rec, U, B, HW)
    written = ~torch.isnan(part[:, :, 0, 0])
    rows_ok = bool(torch.equal(written, go.bn_overlap(U, B, dA.shape[0], BM)))
    got = torch.nan_to_num(part, nan=0.0).sum(1)
    if mode == "lattice":
        go.bn_check_exact(refs)
        return rows_ok, all(go.mismatch("part", got[:, k], refs[k]) is None for k in range(2))
    return rows_ok, all(go.worst_ratio((got[:, k] - refs[k]).abs(), go.sum_bound(B * HW, refs[2 + k])) <= 1.0
                        for k in range(2))


@pytest.mark.parametrize("mode", ["lattice", "real"])
def test_bn_partials_emulation(mode):
    g, z, rec = bn_case(mode)
    dA = g.out_bf16()
    if mode == "lattice":
        v = rec["a"][:, :, None] * torch.arange(-4, 5, dtype=D) + rec["b"][:, :, None]
        assert int((v == 0).sum()) > 0 and int((v[:, [0, 1, 2, 3]] == 0).sum()) == 0   # zeros only where intended
    for order in range(3):
        assert bn_verdict(mode, emu_bn(dA, z, rec, order), dA, z, rec) == (True, True)
    assert go.bn_overlap(3, 64, 576).tolist() == [[True, True, False, False], [False, True, True, False],
                                                  [False, False, True, True]]
    assert go.bn_overlap(1, 48, 144).tolist() == [[True]]


# ------------------------------------------------------------------------------------------ loss epilogue
LE, LU, LB, LN, LK = 3, 2, 16, 64, 128


def loss_case(mode, fmt="bf16", round_y=False, qs=None):
    return go.Loss(go.gemm(mode, fmt, LE * LU * LB, LN, LK, 2, True), LE, LU, LB, 0, True, round_y, qs)


def emu_loss(L: go.Loss, order=0, split=False, round_y=None, t8_from_bf16=False):
    """fp32 emulation of the loss epilogue on the emulated forward."""
    g = L.g
    y = emu_out(g, emu_acc(g, order, split), True).to(F32)
    if L.round_y if round_y is None else round_y:
        y = y.to(BF).to(F32)
    ro = L.rowoff.long()
    perm = torch.randperm(L.M, generator=torch.Generator().manual_seed(order + 7))
    ssum = lambda v: torch.zeros(L.Sn, dtype=F32).index_add_(0, L.stream[perm], v[perm])
    den, denp = ssum(L.rowden[:, 0].to(F32)), ssum(L.rowden[:, 1].to(F32))
    coef = (torch.tensor(L.loss_scale, dtype=F32) * 2 / (float(L.Sn) * den))[L.stream][:, None]
    d, dp = y - L.label[ro].to(F32), y - L.perf[ro].to(F32)
    gf = coef * d
    num, nump = ssum((d * d)[:, torch.randperm(L.N)].sum(1)), ssum((dp * dp).sum(1))
    loss = torch.stack([(num / den).sum() / L.Sn, (nump / denp).sum() / L.Sn])
    dY = gf.to(BF)
    q = torch.tensor(L.qs, dtype=F32)
    e8 = lambda v: (v * q).clamp(-448, 448).to(torch.float8_e4m3fn).to(D)
    return dict(dY=dY.to(D), bg=gf[perm].sum(0).to(D), loss=loss.to(D), den=den.to(D), dY8=e8(gf),
                dYt8=e8(dY.to(F32) if t8_from_bf16 else gf).t(), amax=gf.abs().max().to(D))


def loss_verdict(L: go.Loss, out: dict):
    """(dY, bias gradient, dY8, dYt8 == dY8^T, amax) each equal on the lattice / inside its bound on real data."""
    if L.g.mode == "lattice":
        eq = lambda a, b: go.mismatch("x", a, b) is None
        return (eq(out["dY"], L.dY), eq(out["bg"], L.bias_grad), eq(out["dY8"], L.dY8),
                bool(torch.equal(out["dYt8"], out["dY8"].t())), eq(out["amax"], L.amax) and eq(out["den"], L.den))
    ok = lambda a, ref, bound: go.worst_ratio((a - ref).abs(), bound) <= 1.0
    return (ok(out["dY"], L.gf, L.dY_bound()), ok(out["bg"], L.bias_grad, L.bias_grad_bound()),
            ok(out["dY8"], L.x8(), L.dY8_bound()), bool(torch.equal(out["dYt8"], out["dY8"].t())),
            ok(out["amax"], L.amax, L.err_g.max()) and ok(out["den"], L.den, L.den_bound()))


@pytest.mark.parametrize("round_y", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "e4m3"])
@pytest.mark.parametrize("mode", ["lattice", "real"])
def test_loss_emulation(mode, fmt, round_y):
    L = loss_case(mode, fmt, round_y)
    if mode == "lattice":
        L.check_exact()
        assert int((go.round_bf16(L.g.exact) != L.g.exact).sum()) > 0      # rounding y changes something
    assert float((L.gf * L.qs).abs().max()) > 448                         # some dY8 saturate
    for order, split in ORDERS:
        out = emu_loss(L, order, split)
        assert loss_verdict(L, out) == (True,) * 5, (order, loss_verdict(L, out))
        # the loss pair is not exact, even on the lattice (a division by S = 6 and sums past 2^24): inside its bound
        r = go.worst_ratio((out["loss"] - L.loss).abs(), L.loss_bound())
        assert r <= 1.0, r


# ------------------------------------------------------------------------------------------ mutations
def gemm_verdicts(mut, bias=True, f32=False, variant="scaled"):
    """(rejected on the lattice, rejected by the bound on real data) for a defect ``mut(g, out, acc) -> out``."""
    res = []
    for mode in ("lattice", "real"):
        g = go.gemm(mode, "bf16", I, J, K, 0, bias, variant)
        acc = emu_acc(g, 0, False)
        got = mut(g, emu_out(g, acc, f32), acc)
        if mode == "lattice":
            res.append(go.mismatch("m", got, g.out_f32() if f32 else g.out_bf16()) is not None)
        else:
            res.append(not go.worst_ratio((got - g.out_f32()).abs(), g.bound(f32)) <= 1.0)
    return tuple(res)


def _drop_k_step(g, out, acc):
    P = g.P8.clone()
    P[:T, 64:128] = 0                                   # rows of tile row 0 lose K step 1 ...
    bad = emu_out(g, emu_acc(g, 0, False, P=P), False)
    out = out.clone()
    out[:T, T:] = bad[:T, T:]                           # ... in the output tile (0, 1) only
    return out


def _same_half_twice(g, out, acc):
    P, Q = g.P8.to(F32), g.Q8.to(F32)
    h = g.K // 2
    return emu_out(g, 2 * (P[:, :h] @ Q[:, :h].t()), False)


def _truncate(g, out, acc):
    return emu_out(g, acc, False, trunc=True)


def _bias_shift(g, out, acc):
    return emu_out(g, acc, False, bias=torch.roll(g.bias, 1))


def _fragment_transposed(g, out, acc):
    out = out.clone()
    out[16:32, 32:48] = out[16:32, 32:48].t().clone()
    return out


def _tile_misplaced(g, out, acc):
    out = out.clone()
    out[:T, :T], out[:T, T:] = out[:T, T:].clone(), out[:T, :T].clone()
    return out


# defect -> (the lattice check rejects it, the bounded check rejects it)
GEMM_MUTATIONS = {
    "one K step of 64 dropped in one output tile": (_drop_k_step, (True, True)),
    "both halves of a KS = 2 sum taken from the same half": (_same_half_twice, (True, True)),
    "truncation instead of round-to-nearest-even on the bf16 store": (_truncate, (True, True)),
    "bias shifted by one column": (_bias_shift, (True, True)),
    "one 16 x 16 fragment transposed": (_fragment_transposed, (True, True)),
    "a tile written to its neighbour's place": (_tile_misplaced, (True, True)),
}


@pytest.mark.parametrize("name", list(GEMM_MUTATIONS))
def test_gemm_mutation_is_rejected(name):
    mut, want = GEMM_MUTATIONS[name]
    assert gemm_verdicts(mut) == want, name
    # the clean emulation passes both checks
    assert gemm_verdicts(lambda g, out, acc: out) == (False, False)


def test_bn_mutations_are_rejected():
    # the gate with >= instead of >: only the lattice has a z + b == 0 (real data never hits it: the bound passes)
    for mode, want in (("lattice", (True, False)), ("real", (True, True))):
        g, z, rec = bn_case(mode)
        dA = g.out_bf16()
        assert bn_verdict(mode, emu_bn(dA, z, rec, gate_ge=True), dA, z, rec) == want, mode
    # a straddling tile's upper rows charged to u_lo: the sums are wrong on both, and a row is missing
    for mode in ("lattice", "real"):
        g, z, rec = bn_case(mode)
        dA = g.out_bf16()
        assert bn_verdict(mode, emu_bn(dA, z, rec, charge_lo=True), dA, z, rec) == (False, False), mode


def test_loss_mutations_are_rejected():
    for mode in ("lattice", "real"):
        L = loss_case(mode, "bf16", False)
        # dYt8 quantised from the bf16 dY: a double rounding -- the bytewise dYt8 == dY8^T check rejects it on both
        v = loss_verdict(L, emu_loss(L, t8_from_bf16=True))
        assert v == (True, True, True, False, True), (mode, v)
        # y rounded to bf16 on the path that must not, and not rounded on the path that must: dY and the bias
        # gradient leave the lattice values, and the bounds (the real labels lie near y: |d| << |y|)
        for ry in (False, True):
            Lr = loss_case(mode, "bf16", ry)
            v = loss_verdict(Lr, emu_loss(Lr, round_y=not ry))
            assert v[0] is False and v[1] is False, (mode, ry, v)
