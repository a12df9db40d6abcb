"""The skinny FC forwards (csrc/hip/gemm_skinny.hip, ops.fc.gemm_fwd_skinny / _mix / _rows_f8 / _mix_rows_f8) on a real
MI355X: the four test-time forwards of csrc/hip/gemm.hip for 1 <= M <= 16 output rows, as one weight stream split
over K with an in-launch, fixed-order reduction.

  routed bf16   Y[i, j] = bf16(acc[r_i, j] + b[j]),  r_i = i E + expert[i]
  mix bf16      Y[i, j] = bf16(fma(p2, acc[3 i + 2, j], fma(p1, acc[3 i + 1, j], p0 acc[3 i, j])) + b[j])
  routed e4m3   Y[i, j] = bf16(fma(acc[r_i, j], rs[r_i] cs[j], b[j]))
  mix e4m3      p'_e = p_e rs[3 i + e], Y[i, j] = bf16(fma(fma(p'_2, acc_2, fma(p'_1, acc_1, p'_0 acc_0)), cs[j], b[j]))

Shapes: N = 256, K = 512 (16 column groups, 2 K slices of 4 waves x 64 elements: the smallest K the kernels take),
E = 3, M in {1, 5, 16}; the lattice once more at the real sizes (16, 2048, 4096) and (16, 2048, 8192) (2 and 4 slices
of 4 x 512).  The operands are gemm_oracle.gemm(...)'s for 16 E rows; the calls at M < 16 use their first M E rows.
e4m3: random power-of-two rs / cs with exponents in [-8, 4], as tests/test_gemm_rows_f8_gpu.py builds them.  Every
output is NaN-prefilled with a NaN guard row behind it.

Bounds (tests/test_gemm_mix_gpu.py and tests/test_gemm_rows_f8_gpu.py derive them; nothing new is needed here):
gemm_oracle.fma_term counts K - 1 roundings of partial sums <= S for ANY order and grouping of the K products, so the
split over waves and slices, whose partial tiles are added in fp32, is covered by the same K.  Routed:
bf16_bound(ref, K, S[, align]).  Mix: K' = K + E (the E + 1 roundings of the mix and the bias step), S = sum_e |P_e|
S_e + |b| (e4m3: every S_e and alignment term scaled by rs_e cs, powers of two, so the scaling is exact).
"""
import ctypes

import pytest
import torch

import gemm_oracle as go
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc
from quantum_distributed_machine_learning_ris_channel_estimation_amd.utils.profiling import GraphedStep

pytestmark = pytest.mark.gpu

D, F32, BF, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
NE, MMAX = 3, 16
MS = (1, 5, 16)
SMALL = (256, 512)
REAL_SIZES = ((2048, 4096), (2048, 8192))
FMTS = ("bf16", "e4m3")

_CACHE = {}


def _case(cuda, mode, fmt, N, K, variant="scaled"):
    """Operands and float64 products of one case, computed once and never modified: A (16 E, K), W (N, K) in ``fmt``,
    b (N,) bf16, rs (16 E,), cs (N,) fp32 powers of two (bf16: ones, unused by the kernels); prod / Sabs / align
    (16 E, N) float64 of the UNSCALED product."""
    key = (mode, fmt, N, K, variant)
    if key not in _CACHE:
        g = go.gemm(mode, fmt, MMAX * NE, N, K, 33, True, variant, cuda)
        gen = torch.Generator().manual_seed(2000 + K + N)
        if fmt == "e4m3":
            p2 = lambda n: torch.ldexp(torch.ones(n, dtype=D), torch.randint(-8, 5, (n,), generator=gen)).to(cuda)
        else:
            p2 = lambda n: torch.ones(n, dtype=D, device=cuda)
        rs, cs = p2(MMAX * NE), p2(N)
        dt = F8 if fmt == "e4m3" else BF
        to = lambda t: t.to(F32).to(dt).to(cuda).contiguous()          # (exact: the operands are values of the format)
        zero = torch.zeros(MMAX * NE, N, dtype=D, device=cuda)
        _CACHE[key] = dict(
            g=g, A=to(g.P8), W=to(g.Q8), b=g.bias.to(F32).to(BF).to(cuda).contiguous(), bias=g.bias,
            rs=rs.to(F32).contiguous(), cs=cs.to(F32).contiguous(), rsd=rs, csd=cs,
            prod=g.P8 @ g.Q8.t(), Sabs=g.P8.abs() @ g.Q8.abs().t(),
            align=go.e4m3_align(g.P8, g.Q8) if (mode == "real" and fmt == "e4m3") else zero)
    return _CACHE[key]


def _expert(cuda, M, seed=0):
    return torch.randint(0, NE, (M,), generator=torch.Generator().manual_seed(17 + M + seed)).to(cuda)


def _guarded(cuda, M, N):
    buf = torch.full((M + 1, N), float("nan"), device=cuda, dtype=BF)
    return buf, buf[:M]


def _routed(c, fmt, M, expert, out, A=None, ws=None):
    A = c["A"] if A is None else A
    if fmt == "e4m3":
        return fc.gemm_fwd_skinny_rows_f8(A[:M * NE], c["W"], c["rs"], c["cs"], c["b"], out=out, expert=expert,
                                          n_experts=NE, ws=ws)
    return fc.gemm_fwd_skinny(A[:M * NE], c["W"], c["b"], out=out, expert=expert, n_experts=NE, ws=ws)


def _mix(c, fmt, M, P, out, A=None, ws=None):
    A = c["A"] if A is None else A
    if fmt == "e4m3":
        return fc.gemm_fwd_skinny_mix_rows_f8(A[:M * NE], c["W"], c["rs"], c["cs"], c["b"], P, out=out, ws=ws)
    return fc.gemm_fwd_skinny_mix(A[:M * NE], c["W"], c["b"], P, out=out, ws=ws)


def _routed_ref(c, expert):
    """(ref, S, align) float64 (M, N) of the routed forward (bf16: the scales are ones)."""
    s = go.route(c["rsd"], expert, NE)[:, None] * c["csd"][None, :]
    r = lambda t: go.route(t, expert, NE)
    return r(c["prod"]) * s + c["bias"], r(c["Sabs"]) * s + c["bias"].abs(), r(c["align"]) * s


def _bits(t):
    return t.contiguous().view(torch.int16)


def _onehot(expert):
    P = torch.zeros(expert.numel(), NE, device=expert.device, dtype=F32)
    P[torch.arange(expert.numel(), device=expert.device), expert] = 1.0
    return P


def _weights(cuda):
    """The weight sets of tests/test_gemm_mix_gpu.py at 16 rows; row 7 of ``zero_row`` is all zero."""
    g = torch.Generator().manual_seed(11)
    soft = torch.softmax(4 * torch.randn(MMAX, NE, generator=g), 1)
    half = torch.tensor([0.5, 0.5, 0.0]).repeat(MMAX, 1)
    hot = torch.zeros(MMAX, NE)
    hot[torch.arange(MMAX), torch.randint(0, NE, (MMAX,), generator=g)] = 1.0
    zrow = soft.clone()
    zrow[7] = 0.0
    return {k: v.to(F32).to(cuda).contiguous() for k, v in
            (("softmax", soft), ("half", half), ("onehot", hot), ("zero_row", zrow))}


# ================================================================================ 1. lattice: exact
def _lattice(cuda, fmt, N, K, Ms):
    c = _case(cuda, "lattice", fmt, N, K)
    assert c["g"].n_ties > 0
    fails = []
    for M in Ms:
        expert = _expert(cuda, M)
        ref, _, _ = _routed_ref(c, expert)
        want = go.round_bf16(ref)
        # (the reference alone: one fp32 rounding before the store moves no bf16 result)
        assert torch.equal(go.round_bf16(ref.to(F32).to(D)), want)
        if M == MMAX:
            assert go.bf16_ties(ref) > 0
        buf, Y = _guarded(cuda, M, N)
        _routed(c, fmt, M, expert, Y)
        torch.cuda.synchronize()
        msg = go.mismatch(f"skinny {fmt} N{N} K{K} M{M}", Y.to(D), want)
        if msg:
            fails.append(msg)
        if not bool(torch.isnan(buf[M]).all()):
            fails.append(f"M{M}: guard row written")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
def test_lattice_equals_float64_rounded_to_bf16(cuda, fmt):
    _lattice(cuda, fmt, *SMALL, MS)


@pytest.mark.parametrize("N,K", REAL_SIZES, ids=["P128", "P256"])
@pytest.mark.parametrize("fmt", FMTS)
def test_lattice_at_the_real_sizes(cuda, fmt, N, K):
    _lattice(cuda, fmt, N, K, (MMAX,))


# ================================================================================ 2. real operands: bounded
@pytest.mark.parametrize("fmt", FMTS)
def test_real_routed_within_the_forward_bound(cuda, fmt):
    N, K = SMALL
    fails = []
    for variant in ("scaled", "cancel"):
        c = _case(cuda, "real", fmt, N, K, variant)
        for M in MS:
            expert = _expert(cuda, M)
            ref, S, align = _routed_ref(c, expert)
            buf, Y = _guarded(cuda, M, N)
            _routed(c, fmt, M, expert, Y)
            torch.cuda.synchronize()
            r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K, S, align))
            print(f"ERRBOUND skinny routed {fmt} M{M} {variant} {r:.4f}")
            if not r <= 1.0:
                fails.append(f"{fmt} M{M} {variant}: max err / bound = {r}")
            if not bool(torch.isnan(buf[M]).all()):
                fails.append(f"M{M}: guard row written")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
def test_real_mix_against_float64(cuda, fmt):
    N, K = SMALL
    c = _case(cuda, "real", fmt, N, K)
    sc = c["rsd"].view(MMAX, NE, 1) * c["csd"].view(1, 1, N)
    v3 = lambda t: t.view(MMAX, NE, N) * sc
    prod, Sabs, align = v3(c["prod"]), v3(c["Sabs"]), v3(c["align"])
    fails = []
    for name, P16 in _weights(cuda).items():
        for M in (MMAX, 8):      # (8: past the zero row, short of the tile)
            P = P16[:M].contiguous()
            buf, Y = _guarded(cuda, M, N)
            _mix(c, fmt, M, P, Y)
            torch.cuda.synchronize()
            Pd = P.to(D)
            ref = (Pd[:, :, None] * prod[:M]).sum(1) + c["bias"]
            S = (Pd.abs()[:, :, None] * Sabs[:M]).sum(1) + c["bias"].abs()
            al = (Pd.abs()[:, :, None] * align[:M]).sum(1)
            r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K + NE, S, al))
            print(f"ERRBOUND skinny mix {fmt} M{M} {name} {r:.4f}")
            if not r <= 1.0:
                fails.append(f"{fmt} M{M} {name}: max err / bound = {r}")
            if not bool(torch.isnan(buf[M]).all()):
                fails.append(f"{fmt} M{M} {name}: guard row written")
            if name == "zero_row" and not torch.equal(_bits(Y[7]), _bits(c["b"])):
                fails.append(f"{fmt} M{M} zero_row: an all-zero weight row must give the bias itself")
    assert not fails, "\n".join(fails)


# ================================================================================ 3. mix, one-hot == routed
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M", MS)
def test_mix_one_hot_equals_the_skinny_routed_forward_bit_for_bit(cuda, fmt, M):
    N, K = SMALL
    c = _case(cuda, "real", fmt, N, K)
    expert = _expert(cuda, M, 2)
    buf, Y = _guarded(cuda, M, N)
    _mix(c, fmt, M, _onehot(expert), Y)
    bufr, Yr = _guarded(cuda, M, N)
    _routed(c, fmt, M, expert, Yr)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Y).any()) and not bool(torch.isnan(Yr).any())
    assert torch.equal(_bits(Y), _bits(Yr))
    assert bool(torch.isnan(buf[M]).all()) and bool(torch.isnan(bufr[M]).all()), "guard row written"


# ================================================================================ 4. row independence
@pytest.mark.parametrize("form", ["routed", "mix"])
@pytest.mark.parametrize("fmt", FMTS)
def test_row_0_does_not_depend_on_m_or_on_the_other_rows(cuda, fmt, form):
    N, K = SMALL
    c = _case(cuda, "real", fmt, N, K)
    expert = _expert(cuda, MMAX, 3)
    P = _weights(cuda)["softmax"]
    run = lambda M, e, p, A=None: (_routed(c, fmt, M, e[:M].contiguous(), _guarded(cuda, M, N)[1], A) if form == "routed"
                                   else _mix(c, fmt, M, p[:M].contiguous(), _guarded(cuda, M, N)[1], A))
    y16 = run(MMAX, expert, P)
    y1 = run(1, expert, P)
    # other rows: new operands (NaN among them), new experts, new weights
    A2 = c["A"].clone()
    A2v = A2.view(torch.uint8) if fmt == "e4m3" else A2
    A2v[NE:] = A2v[NE:].flip(0)
    nanrow = torch.full((K,), float("nan"), device=cuda).to(A2.dtype)
    (A2v[2 * NE + 1]).copy_(nanrow.view(torch.uint8) if fmt == "e4m3" else nanrow)
    e2 = (expert + 1) % NE
    e2[0] = expert[0]
    P2 = P.flip(0).contiguous()
    P2[0] = P[0]
    y16b = run(MMAX, e2, P2, A2)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y16[0]).any())
    assert torch.equal(_bits(y1[0]), _bits(y16[0])), "row 0 at M = 1 differs from row 0 at M = 16"
    assert torch.equal(_bits(y16b[0]), _bits(y16[0])), "row 0 changed with the other rows' operands"
    assert not torch.equal(_bits(y16b[1:]), _bits(y16[1:]))     # (the other rows did change)


# ================================================================================ 5. state and determinism
@pytest.mark.parametrize("form", ["routed", "mix"])
@pytest.mark.parametrize("fmt", FMTS)
def test_eager_twice_graph_replays_and_lds_poison(cuda, fmt, form):
    N, K = SMALL
    M = 5
    c = _case(cuda, "real", fmt, N, K)
    expert = _expert(cuda, M, 4)
    P = _weights(cuda)["softmax"][:M].contiguous()
    ws = fc.gemm_skinny_workspace(N, K, cuda, cached=False)
    A = c["A"][:M * NE].clone()

    def call(out):
        return _routed(c, fmt, M, expert, out, A, ws) if form == "routed" else _mix(c, fmt, M, P, out, A, ws)

    y0 = call(_guarded(cuda, M, N)[1]).clone()
    y1 = call(_guarded(cuda, M, N)[1]).clone()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y0).any()) and torch.equal(_bits(y0), _bits(y1))

    # one captured call, replayed with A rewritten: each replay equals an eager call on the same A (a ticket or a
    # slab that survives a call shows here)
    buf, Yg = _guarded(cuda, M, N)
    step = GraphedStep(lambda: call(Yg), warmup=1)
    step.capture()
    torch.cuda.synchronize()
    Av = A.view(torch.uint8) if fmt == "e4m3" else A
    src = c["A"].view(torch.uint8) if fmt == "e4m3" else c["A"]
    for rep in range(3):
        Av.copy_(src[(rep + 1) * NE:(rep + 1) * NE + M * NE])
        Yg.fill_(float("nan"))
        torch.cuda.synchronize()
        step()
        torch.cuda.synchronize()
        got = Yg.clone()
        want = call(_guarded(cuda, M, N)[1])
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got).any())
        assert torch.equal(_bits(got), _bits(want)), f"replay {rep}"
        assert bool(torch.isnan(buf[M]).all()), "guard row written"
    step.close()     # (the executable is parked until exit: utils/profiling.py's rule)

    # LDS poisoning: bit-identical to the clean call
    Av.copy_(src[:M * NE])
    try:
        for pattern in (0xFFFFFFFF, 0x7F7F7F7F):
            nat.set_lds_poison(pattern)
            yp = call(_guarded(cuda, M, N)[1])
            torch.cuda.synchronize()
            assert torch.equal(_bits(yp), _bits(y0)), hex(pattern)
    finally:
        nat.set_lds_poison(None)


# ================================================================================ 6. refusals
_p, _i = ctypes.c_void_p, ctypes.c_int


def _raw(cuda, entry, M, N, K, E, ws_null=False):
    """The raw entry point's status on (M, N, K, E), with operands large enough for any of the cases; Y guarded."""
    f8 = entry.endswith("f8")
    rows = 17 * 4
    dt = F8 if f8 else BF
    A = torch.ones(rows, 1024, device=cuda).to(dt)
    W = torch.ones(272, 1024, device=cuda).to(dt)
    b = torch.ones(272, device=cuda, dtype=BF)
    rs, cs = torch.ones(rows, device=cuda), torch.ones(272, device=cuda)
    P = torch.full((17, 4), 0.25, device=cuda)
    ex = torch.zeros(17, dtype=torch.int64, device=cuda)
    ws = fc.gemm_skinny_workspace(256, 512, cuda, cached=False)
    buf = torch.full((18, 272), float("nan"), device=cuda, dtype=BF)
    pw = None if ws_null else nat.ptr(ws)
    st = nat.stream_ptr(cuda)
    lib = nat.hip_lib()
    if entry == "routed":
        f = nat.fn(lib, "qd_gemm_fwd_skinny", [_p, _p, _p, _p, _i, _i, _i, _p, _i, _p, _p])
        s = f(nat.ptr(A), nat.ptr(W), nat.ptr(b), nat.ptr(buf), M, N, K, nat.ptr(ex), E, pw, st)
    elif entry == "mix":
        f = nat.fn(lib, "qd_gemm_fwd_skinny_mix", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
        s = f(nat.ptr(A), nat.ptr(W), nat.ptr(b), nat.ptr(P), nat.ptr(buf), M, N, K, E, pw, st)
    elif entry == "routed_f8":
        f = nat.fn(lib, "qd_gemm_fwd_skinny_rows_f8", [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _i, _p, _p])
        s = f(nat.ptr(A), nat.ptr(W), nat.ptr(rs), nat.ptr(cs), nat.ptr(b), nat.ptr(buf), M, N, K, nat.ptr(ex), E, pw,
              st)
    else:
        f = nat.fn(lib, "qd_gemm_fwd_skinny_mix_rows_f8", [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
        s = f(nat.ptr(A), nat.ptr(W), nat.ptr(rs), nat.ptr(cs), nat.ptr(b), nat.ptr(P), nat.ptr(buf), M, N, K, E, pw,
              st)
    torch.cuda.synchronize()
    return s, buf


REFUSALS = [("M=0", 0, 256, 512, 3, False), ("M=17", 17, 256, 512, 3, False), ("N=264", 5, 264, 512, 3, False),
            ("N=0", 5, 0, 512, 3, False), ("K=256", 5, 256, 256, 3, False), ("K=768", 5, 256, 768, 3, False),
            ("K=0", 5, 256, 0, 3, False), ("null ws", 5, 256, 512, 3, True)]


@pytest.mark.parametrize("what,M,N,K,E,ws_null", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("entry", ["routed", "mix", "routed_f8", "mix_f8"])
def test_refusals_leave_y_untouched(cuda, entry, what, M, N, K, E, ws_null):
    if what not in ("null ws",):
        assert not fc.gemm_fwd_skinny_ok(M, N, K, entry.endswith("f8"))
    s, buf = _raw(cuda, entry, M, N, K, E, ws_null)
    assert s != 0, "accepted"
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("entry", ["mix", "mix_f8"])
def test_the_mix_refuses_other_expert_counts(cuda, entry, E):
    s, buf = _raw(cuda, entry, 5, 256, 512, E)
    assert s != 0, "accepted"
    assert bool(torch.isnan(buf).all())
    # and the Python layer raises before any launch
    c = _case(cuda, "real", "e4m3" if entry == "mix_f8" else "bf16", *SMALL)
    bufy, Y = _guarded(cuda, 5, SMALL[0])
    with pytest.raises(ValueError):
        _mix(c, "e4m3" if entry == "mix_f8" else "bf16", 5, torch.full((5, E), 1.0 / E, device=cuda), Y)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufy).all())


def test_the_python_layer_raises_value_error_outside_the_rules(cuda):
    c = _case(cuda, "real", "bf16", *SMALL)
    N, K = SMALL
    buf = torch.full((18, N), float("nan"), device=cuda, dtype=BF)
    A17 = torch.zeros(17 * NE, K, device=cuda, dtype=BF)
    with pytest.raises(ValueError):
        fc.gemm_fwd_skinny(A17, c["W"], c["b"], out=buf[:17], expert=torch.zeros(17, dtype=torch.int64, device=cuda),
                           n_experts=NE)
    with pytest.raises(ValueError):      # (no expert indices with 3 experts)
        fc.gemm_fwd_skinny(c["A"][:5 * NE], c["W"], c["b"], out=buf[:5], n_experts=NE)
    with pytest.raises(ValueError):
        fc.gemm_fwd_skinny(c["A"][:5, :256].contiguous(), c["W"][:, :256].contiguous(), c["b"], out=buf[:5])
    with pytest.raises(ValueError):
        fc.gemm_skinny_workspace(264, 512, cuda)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert fc.gemm_fwd_skinny_ok(16, 2048, 4096) and fc.gemm_fwd_skinny_ok(1, 2048, 8192, True)


def test_a_single_expert_needs_no_indices(cuda):
    """E == 1 with ``expert`` null: plain rows, equal to the routed call with all-zero indices."""
    c = _case(cuda, "real", "bf16", *SMALL)
    N, K = SMALL
    M = 5
    buf, Y = _guarded(cuda, M, N)
    fc.gemm_fwd_skinny(c["A"][:M], c["W"], c["b"], out=Y)
    Yz = fc.gemm_fwd_skinny(c["A"][:M], c["W"], c["b"], out=_guarded(cuda, M, N)[1],
                            expert=torch.zeros(M, dtype=torch.int64, device=cuda), n_experts=1)
    torch.cuda.synchronize()
    ref = c["prod"][:M] + c["bias"]
    r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K, c["Sabs"][:M] + c["bias"].abs()))
    assert r <= 1.0 and torch.equal(_bits(Y), _bits(Yz)) and bool(torch.isnan(buf[M]).all())
