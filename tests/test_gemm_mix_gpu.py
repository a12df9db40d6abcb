"""The mixing epilogue of the inference FC forward (csrc/hip/gemm.hip EPI_MIX, ops.fc.gemm_fwd_mix) on a real MI355X:

  Y[i, j] = bf16(fma(P[i, 2], acc[3 i + 2, j], fma(P[i, 1], acc[3 i + 1, j], P[i, 0] acc[3 i, j])) + bias[j])

1. one-hot weights equal the expert-routed forward bit for bit (1 acc + 0 finite is exact, and a row's K order does
   not depend on the rows that share its tile);
2. general weights against the float64 reference within a derived per-element bound;
3. refusals raise before any launch and leave Y untouched.

Shapes: N = 256, K = 320 (five K steps, an odd count), E = 3 -- the routed-forward test's sizes; M = 48 (one 144-row
tile of the dense product) and 576 (four).  Y is NaN-prefilled and has a NaN guard row behind it.

The bound.  S_e = |A_e| |W|^T, S = sum_e |P_e| S_e + |b|.  acc_e is an fp32 accumulation of K exact products: K - 1
roundings of partial sums <= S_e (gemm_oracle.fma_term's argument), i.e. |acc_e - A_e W^T| <= (K - 1) eps S_e, which
the weights scale to (K - 1) eps |P_e| S_e.  The mix adds one rounding per term -- fl(P_0 acc_0), then one per fma --
each of a partial sum <= sum_e |P_e| S_e, and the bias addition one more on a value <= S: E + 1 roundings.  (P is an
fp32 INPUT: the reference uses its values exactly.)  Together (K + E) eps S <= fma_term(K + E, S) = (K + E + 2) eps S,
so the helper's form covers it with K' = K + E: the bound is gemm_oracle.bf16_bound(ref, K + E, S), the store being one
bf16 rounding of that fp32 value.

Partial tiles.  No forward tile of gemm.hip takes a partial tile -- the routed forward at cfg 8 needs M % 144 == 0
like cfg 0 (qd_gemm_fwd_ok) -- and the mix follows the routed forward's rules at the same cfg, so M = 50 and M = 100
are refused at both cfgs: they are cases of test 3, not of tests 1 and 2.
"""
import pytest
import torch

import gemm_oracle as go
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc

pytestmark = pytest.mark.gpu

D, F32, BF = torch.float64, torch.float32, torch.bfloat16
MMAX, N, K, NE = 576, 256, 320, 3
CFGS = (0, 8)


def _operands(cuda):
    """The routed-forward test's operands (cached by gemm_oracle.gemm): A (MMAX NE, K), W (N, K), bias (N)."""
    g = go.gemm("real", "bf16", MMAX * NE, N, K, 8, True, "scaled", cuda)
    to = lambda t: t.to(F32).to(BF).to(cuda).contiguous()   # (exact: the operands are bf16 values)
    return g, to(g.P8), to(g.Q8), to(g.bias)


def _guarded(cuda, M):
    """Y (M, N) NaN-prefilled, a view of a buffer with one NaN guard row behind it."""
    buf = torch.full((M + 1, N), float("nan"), device=cuda, dtype=BF)
    return buf, buf[:M]


def _onehot(expert):
    P = torch.zeros(expert.numel(), NE, device=expert.device, dtype=F32)
    P[torch.arange(expert.numel(), device=expert.device), expert] = 1.0
    return P


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M", [48, 576])
def test_one_hot_weights_equal_the_routed_forward_bit_for_bit(cuda, cfg, M):
    _, A, W, b = _operands(cuda)
    expert = torch.randint(0, NE, (M,), generator=torch.Generator().manual_seed(5 + M)).to(cuda)
    buf, Y = _guarded(cuda, M)
    fc.gemm_fwd_mix(A, W, b, _onehot(expert), out=Y, cfg=cfg)
    # the routed forward tiles its M OUTPUT rows: run it on the first whole tile(s) and compare the first M rows
    Mr = -(-M // 144) * 144
    er = torch.zeros(Mr, device=cuda, dtype=torch.int64)
    er[:M] = expert
    Yr = fc.gemm_fwd(A, W, b, out=torch.full((Mr, N), float("nan"), device=cuda, dtype=BF), cfg=cfg, expert=er,
                     n_experts=NE)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Y).any())
    assert torch.equal(Y.view(torch.int16), Yr[:M].view(torch.int16))
    assert bool(torch.isnan(buf[M]).all()), "guard row written"


def _weights(cuda):
    g = torch.Generator().manual_seed(11)
    soft = torch.softmax(4 * torch.randn(MMAX, NE, generator=g), 1)
    half = torch.tensor([0.5, 0.5, 0.0]).repeat(MMAX, 1)
    hot = torch.zeros(MMAX, NE)
    hot[torch.arange(MMAX), torch.randint(0, NE, (MMAX,), generator=g)] = 1.0
    zrow = soft.clone()
    zrow[77] = 0.0
    return {k: v.to(F32).to(cuda).contiguous() for k, v in
            (("softmax", soft), ("half", half), ("onehot", hot), ("zero_row", zrow))}


@pytest.mark.parametrize("cfg", CFGS)
def test_general_weights_against_float64(cuda, cfg):
    g, A, W, b = _operands(cuda)
    prod = (g.P @ g.Q.t()).view(MMAX, NE, N)                  # float64, from the bf16 operands
    Sabs = (g.P.abs() @ g.Q.abs().t()).view(MMAX, NE, N)
    fails = []
    for name, P in _weights(cuda).items():
        buf, Y = _guarded(cuda, MMAX)
        fc.gemm_fwd_mix(A, W, b, P, out=Y, cfg=cfg)
        torch.cuda.synchronize()
        Pd = P.to(D)
        ref = (Pd[:, :, None] * prod).sum(1) + g.bias
        S = (Pd.abs()[:, :, None] * Sabs).sum(1) + g.bias.abs()
        r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K + NE, S))
        print(f"ERRBOUND mix cfg{cfg} {name} {r:.4f}")
        if not r <= 1.0:
            fails.append(f"{name}: max err / bound = {r}")
        if not bool(torch.isnan(buf[MMAX]).all()):
            fails.append(f"{name}: guard row written")
        if name == "zero_row" and not torch.equal(Y[77].view(torch.int16), b.view(torch.int16)):
            fails.append("zero_row: an all-zero weight row must give the bias itself")
    assert not fails, "\n".join(fails)


REFUSALS = [("E=2", 72, 2, 0, K), ("E=4", 36, 4, 0, K), ("E=2 cfg8", 72, 2, 8, K), ("E=4 cfg8", 36, 4, 8, K),
            ("cfg 5", 576, 3, 5, 256), ("cfg 1", 576, 3, 1, K),
            ("M=50 cfg0", 50, 3, 0, K), ("M=100 cfg0", 100, 3, 0, K), ("M=50 cfg8", 50, 3, 8, K),
            ("M=100 cfg8", 100, 3, 8, K), ("K=96", 48, 3, 0, 96)]


@pytest.mark.parametrize("what,M,E,cfg,Kc", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_y_untouched(cuda, what, M, E, cfg, Kc):
    """E != 3, the direct-A tile (cfg 5; K = 256, a shape it would otherwise tile), a tile the mix does not
    instantiate (cfg 1), and shapes the cfg does not tile (M E not a multiple of 144; K not a multiple of 64)."""
    _, A, W, _ = _operands(cuda)
    A, W = A[:, :Kc].contiguous(), W[:, :Kc].contiguous()
    buf, Y = _guarded(cuda, M)
    P = torch.full((M, E), 1.0 / E, device=cuda, dtype=F32)
    with pytest.raises(RuntimeError):
        fc.gemm_fwd_mix(A, W, None, P, out=Y, cfg=cfg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
