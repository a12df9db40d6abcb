"""The e4m3 test-time forwards with per-row and per-column power-of-two scales (csrc/hip/gemm.hip
qd_gemm_fwd_rows_f8 / qd_gemm_fwd_mix_rows_f8, ops.fc.gemm_fwd_rows_f8 / gemm_fwd_mix_rows_f8) on a real MI355X:

  routed  Y[i, j] = bf16(fma(acc[r_i, j], rs[r_i] cs[j], b[j])),  r_i = i E + expert[i]
  mixed   Y[i, j] = bf16(fma(m, cs[j], b[j])),  m = fma(p'_2, acc_2, fma(p'_1, acc_1, p'_0 acc_0)),  p'_e = P[i, e] rs[3 i + e]

acc being the fp32 accumulation of the e4m3 products that the three forward tiles produce (cfg 0: FwdA8, 1: FwdM8,
2: FwdM8P with producer waves).

Shapes: M = 144 and 576 output rows (one and four tiles), N = 256 (two tile columns), E = 3; K = 128, 256, 512 at
cfg 0 and 256, 512 at cfgs 1 and 2 (the MX MFMA takes K in steps of 256) -- tests/test_gemm_exact_gpu.py::test_fwd_f8's
K sweep.  The operands are gemm_oracle.gemm(mode, "e4m3", M E, N, K, ..., bias=True)'s e4m3 values P8 / Q8 (its
per-tensor scales are not used); rs (M E,) and cs (N,) are random powers of two with exponents in [-8, 4].  Every
output buffer is NaN-prefilled.

The reference is float64: ref = (P8 Q8^T)[r, j] rs[r] cs[j] + b[j].  The scales are powers of two, so scaling is exact
and commutes with every rounding of the accumulation: the bound of the unscaled product holds scaled by rs[r] cs[j].

  lattice   integer operands whose every partial sum is exact in fp32: acc IS the integer sum, the fma is the one
            fp32 rounding of ref and the store the bf16 rounding of that.  Y must equal round_bf16(ref) bit for bit
            (the test first checks, on the reference alone, that rounding through fp32 does not move any bf16 result).
  real      |Y - ref| <= gemm_oracle.bf16_bound(ref, K, S, align) with S = (|P8| |Q8|^T) rs cs + |b| and the e4m3
            alignment term scaled alike -- Gemm.bound's form.  With |acc| <= K 448^2 < 2^27 and exponents in
            [-16, 8] nothing under- or overflows.
  mixed     the bound of tests/test_gemm_mix_gpu.py: K' = K + E roundings (the E + 1 of the mix and the final fma on
            top of the accumulation), S = sum_e |P_e| rs_e S_e cs + |b|, the alignment term summed the same way.
"""
import ctypes

import pytest
import torch

import gemm_oracle as go
from test_gemm_mix_gpu import _weights
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc

pytestmark = pytest.mark.gpu

D, F32, BF, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
MMAX, N, NE = 576, 256, 3
MS = (144, 576)
CFGS = (0, 1, 2)


def _ks(cfg):
    return (128, 256, 512) if cfg == 0 else (256, 512)


_CACHE = {}


def _case(cuda, mode, K, variant="scaled"):
    """Operands and float64 products of one (mode, K), computed once: A8 (MMAX E, K), W8 (N, K) e4m3, b (N,) bf16,
    rs (MMAX E,), cs (N,) fp32 powers of two; prod / Sabs / align (MMAX E, N) float64 of the UNSCALED product."""
    key = (mode, K, variant)
    if key not in _CACHE:
        g = go.gemm(mode, "e4m3", MMAX * NE, N, K, 21, True, variant, cuda)
        gen = torch.Generator().manual_seed(1000 + K)
        p2 = lambda n: torch.ldexp(torch.ones(n, dtype=D), torch.randint(-8, 5, (n,), generator=gen)).to(cuda)
        rs, cs = p2(MMAX * NE), p2(N)
        to8 = lambda t: t.to(F32).to(F8).to(cuda).contiguous()           # (exact: the operands are e4m3 values)
        _CACHE[key] = dict(
            A8=to8(g.P8), W8=to8(g.Q8), b=g.bias.to(F32).to(BF).to(cuda).contiguous(), bias=g.bias,
            rs=rs.to(F32).contiguous(), cs=cs.to(F32).contiguous(), rsd=rs, csd=cs,
            prod=g.P8 @ g.Q8.t(), Sabs=g.P8.abs() @ g.Q8.abs().t(),
            align=go.e4m3_align(g.P8, g.Q8) if mode == "real" else torch.zeros(MMAX * NE, N, dtype=D, device=cuda))
    return _CACHE[key]


def _expert(cuda, M, seed=0):
    return torch.randint(0, NE, (M,), generator=torch.Generator().manual_seed(7 + M + seed)).to(cuda)


def _nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda, dtype=BF)


def _guarded(cuda, M):
    buf = _nan(cuda, M + 1, N)
    return buf, buf[:M]


def _routed_ref(c, expert):
    """(ref, S, align) float64 (M, N) of the routed forward."""
    s = go.route(c["rsd"], expert, NE)[:, None] * c["csd"][None, :]
    r = lambda t: go.route(t, expert, NE)
    return r(c["prod"]) * s + c["bias"], r(c["Sabs"]) * s + c["bias"].abs(), r(c["align"]) * s


# ================================================================================ 1. lattice: exact
@pytest.mark.parametrize("cfg", CFGS)
def test_lattice_routed_equals_float64_rounded_to_bf16(cuda, cfg):
    fails = []
    for K in _ks(cfg):
        c = _case(cuda, "lattice", K)
        for M in MS:
            expert = _expert(cuda, M)
            ref, _, _ = _routed_ref(c, expert)
            want = go.round_bf16(ref)
            # (the operands' own exactness: one fp32 rounding before the store changes no bf16 result, and the sums
            # reach bf16 ties)
            assert torch.equal(go.round_bf16(ref.to(F32).to(D)), want) and go.bf16_ties(ref) > 0
            Y = _nan(cuda, M, N)
            fc.gemm_fwd_rows_f8(c["A8"], c["W8"], c["rs"], c["cs"], c["b"], out=Y, cfg=cfg, expert=expert,
                                n_experts=NE)
            msg = go.mismatch(f"rows_f8 cfg{cfg} K{K} M{M}", Y.to(D), want)
            if msg:
                fails.append(msg)
    torch.cuda.synchronize()
    assert not fails, "\n".join(fails)


# ================================================================================ 2. real operands: bounded
@pytest.mark.parametrize("cfg", CFGS)
def test_real_routed_within_the_e4m3_forward_bound(cuda, cfg):
    fails = []
    for K in _ks(cfg):
        for variant in ("scaled", "cancel"):
            c = _case(cuda, "real", K, variant)
            for M in MS:
                expert = _expert(cuda, M)
                ref, S, align = _routed_ref(c, expert)
                Y = _nan(cuda, M, N)
                fc.gemm_fwd_rows_f8(c["A8"], c["W8"], c["rs"], c["cs"], c["b"], out=Y, cfg=cfg, expert=expert,
                                    n_experts=NE)
                r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K, S, align))
                print(f"ERRBOUND rows_f8 cfg{cfg} K{K} M{M} {variant} {r:.4f}")
                if not r <= 1.0:
                    fails.append(f"cfg{cfg} K{K} M{M} {variant}: max err / bound = {r}")
    assert not fails, "\n".join(fails)


# ================================================================================ 3. routed == gathered
@pytest.mark.parametrize("cfg", CFGS)
def test_routed_is_bit_identical_to_the_gathered_rows(cuda, cfg):
    for K in _ks(cfg):
        c = _case(cuda, "real", K)
        for M in MS:
            expert = _expert(cuda, M, 1)
            Y = _nan(cuda, M, N)
            fc.gemm_fwd_rows_f8(c["A8"], c["W8"], c["rs"], c["cs"], c["b"], out=Y, cfg=cfg, expert=expert,
                                n_experts=NE)
            Ag = go.route(c["A8"].view(torch.uint8), expert, NE).contiguous().view(F8)
            rg = go.route(c["rs"], expert, NE).contiguous()
            Yg = fc.gemm_fwd_rows_f8(Ag, c["W8"], rg, c["cs"], c["b"], out=_nan(cuda, M, N), cfg=cfg)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(Y).any())
            assert torch.equal(Y.view(torch.int16), Yg.view(torch.int16)), (cfg, K, M)


# ================================================================================ 4. mix, one-hot == routed
def _onehot(expert):
    P = torch.zeros(expert.numel(), NE, device=expert.device, dtype=F32)
    P[torch.arange(expert.numel(), device=expert.device), expert] = 1.0
    return P


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M", [48, 576])
def test_mix_one_hot_equals_the_routed_forward_bit_for_bit(cuda, cfg, M):
    for K in _ks(cfg):
        c = _case(cuda, "real", K)
        expert = _expert(cuda, M, 2)
        buf, Y = _guarded(cuda, M)
        fc.gemm_fwd_mix_rows_f8(c["A8"][:M * NE], c["W8"], c["rs"][:M * NE], c["cs"], c["b"], _onehot(expert), out=Y,
                                cfg=cfg)
        Mr = -(-M // 144) * 144          # (the routed forward tiles its M OUTPUT rows)
        er = torch.zeros(Mr, device=cuda, dtype=torch.int64)
        er[:M] = expert
        Yr = fc.gemm_fwd_rows_f8(c["A8"], c["W8"], c["rs"], c["cs"], c["b"], out=_nan(cuda, Mr, N), cfg=cfg, expert=er,
                                 n_experts=NE)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(Y).any())
        assert torch.equal(Y.view(torch.int16), Yr[:M].view(torch.int16)), (cfg, K, M)
        assert bool(torch.isnan(buf[M]).all()), "guard row written"


# ================================================================================ 5. mix, general weights
@pytest.mark.parametrize("cfg", CFGS)
def test_mix_general_weights_against_float64(cuda, cfg):
    fails = []
    for K in _ks(cfg):
        c = _case(cuda, "real", K)
        sc = c["rsd"].view(MMAX, NE, 1) * c["csd"].view(1, 1, N)
        v3 = lambda t: t.view(MMAX, NE, N) * sc
        prod, Sabs, align = v3(c["prod"]), v3(c["Sabs"]), v3(c["align"])
        for name, P in _weights(cuda).items():
            buf, Y = _guarded(cuda, MMAX)
            fc.gemm_fwd_mix_rows_f8(c["A8"], c["W8"], c["rs"], c["cs"], c["b"], P, out=Y, cfg=cfg)
            torch.cuda.synchronize()
            Pd = P.to(D)
            ref = (Pd[:, :, None] * prod).sum(1) + c["bias"]
            S = (Pd.abs()[:, :, None] * Sabs).sum(1) + c["bias"].abs()
            al = (Pd.abs()[:, :, None] * align).sum(1)
            r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K + NE, S, al))
            print(f"ERRBOUND mix_rows_f8 cfg{cfg} K{K} {name} {r:.4f}")
            if not r <= 1.0:
                fails.append(f"K{K} {name}: max err / bound = {r}")
            if not bool(torch.isnan(buf[MMAX]).all()):
                fails.append(f"K{K} {name}: guard row written")
            if name == "zero_row" and not torch.equal(Y[77].view(torch.int16), c["b"].view(torch.int16)):
                fails.append(f"K{K} zero_row: an all-zero weight row must give the bias itself")
    assert not fails, "\n".join(fails)


# ================================================================================ 6. refusals
def _refusal_operands(cuda, rows, K):
    c = _case(cuda, "real", 256)
    return c["A8"][:rows, :K].contiguous(), c["W8"][:, :K].contiguous(), c["rs"][:rows].contiguous(), c["cs"], c["b"]


MIX_REFUSALS = [("E=2", 72, 2, 0, 256), ("E=4", 36, 4, 2, 256), ("M=50", 50, 3, 0, 256), ("M=50 cfg2", 50, 3, 2, 256),
                ("K=96", 48, 3, 0, 96), ("cfg1 K=128", 48, 3, 1, 128), ("cfg2 K=128", 48, 3, 2, 128),
                ("cfg 3", 48, 3, 3, 256)]


@pytest.mark.parametrize("what,M,E,cfg,K", MIX_REFUSALS, ids=[r[0] for r in MIX_REFUSALS])
def test_mix_refusals_leave_y_untouched(cuda, what, M, E, cfg, K):
    A8, W8, rs, cs, b = _refusal_operands(cuda, M * E, K)
    buf, Y = _guarded(cuda, M)
    P = torch.full((M, E), 1.0 / E, device=cuda, dtype=F32)
    with pytest.raises(RuntimeError):
        fc.gemm_fwd_mix_rows_f8(A8, W8, rs, cs, b, P, out=Y, cfg=cfg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


ROUTED_REFUSALS = [("M=50", 50, 0, 256), ("M=50 cfg2", 50, 2, 256), ("K=96", 144, 0, 96), ("cfg1 K=128", 144, 1, 128),
                   ("cfg2 K=128", 144, 2, 128), ("cfg 3", 144, 3, 256)]


@pytest.mark.parametrize("what,M,cfg,K", ROUTED_REFUSALS, ids=[r[0] for r in ROUTED_REFUSALS])
@pytest.mark.parametrize("routed", [True, False])
def test_routed_refusals_leave_y_untouched(cuda, what, M, cfg, K, routed):
    A8, W8, rs, cs, b = _refusal_operands(cuda, M * NE if routed else M, K)
    buf, Y = _guarded(cuda, M)
    with pytest.raises(RuntimeError):
        if routed:
            fc.gemm_fwd_rows_f8(A8, W8, rs, cs, b, out=Y, cfg=cfg, expert=_expert(cuda, M), n_experts=NE)
        else:
            fc.gemm_fwd_rows_f8(A8, W8, rs, cs, b, out=Y, cfg=cfg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize("null", ["rs", "cs"])
@pytest.mark.parametrize("entry", ["rows", "mix"])
def test_a_null_scale_pointer_is_refused_by_the_raw_entry_point(cuda, entry, null):
    _p, _i = ctypes.c_void_p, ctypes.c_int
    M, K = 144, 256
    A8, W8, rs, cs, b = _refusal_operands(cuda, M * NE, K)
    buf, Y = _guarded(cuda, M)
    prs = None if null == "rs" else nat.ptr(rs)
    pcs = None if null == "cs" else nat.ptr(cs)
    st = nat.stream_ptr(cuda)
    if entry == "rows":
        f = nat.fn(nat.hip_lib(), "qd_gemm_fwd_rows_f8", [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i, _p])
        status = f(nat.ptr(A8), nat.ptr(W8), prs, pcs, nat.ptr(b), nat.ptr(Y), M, N, K, 0, None, 0, st)
    else:
        P = torch.full((M, NE), 1.0 / NE, device=cuda, dtype=F32)
        f = nat.fn(nat.hip_lib(), "qd_gemm_fwd_mix_rows_f8", [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p])
        status = f(nat.ptr(A8), nat.ptr(W8), prs, pcs, nat.ptr(b), nat.ptr(P), nat.ptr(Y), M, N, K, NE, 0, st)
    with pytest.raises(RuntimeError):
        nat.check(status, entry)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
