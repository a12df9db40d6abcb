"""The FC GEMM kernels of csrc/hip/gemm.hip against the float64 oracle of tests/gemm_oracle.py, on a real MI355X:
exactly (torch.equal) on small-integer lattice operands, and element by element within derived bounds on real-valued
operands (gemm_oracle.f32_bound / bf16_bound / sum_bound / Loss.*_bound, derived there; nothing is masked).

Every output buffer is NaN-prefilled (0xFF bytes for e4m3), so an element a kernel does not write fails the
comparison.  Shapes come from the per-cfg tile tables below, read off gemm.hip's ``Geo`` aliases; each case first
asserts that the kernel's own ``qd_gemm_*_ok`` predicate accepts it.  The K sweep of one (entry, cfg) runs inside one
test: K / 64 = 1 .. 5 covers a K loop shorter than, equal to and longer than the 3- and 4-stage rings, the peeled
tails and the producer waves' barrier counts; the loss epilogue on cfg 8 adds K / 64 = 21 and 22, where its label
prefetch stops being partial.  The references are computed in float64 on the GPU, once per shape (gemm_oracle.gemm
caches them).  Each bounded comparison prints its achieved max(err / bound) as ``ERRBOUND <what> <case> <ratio>``.
The e4m3 bounds carry one term more than the bf16 ones: the e4m3 MFMAs truncate a product 14 bits below the largest
one beside it (gemm_oracle.fma_term; pinned here by test_e4m3_mfma_keeps_14_bits_below_the_largest_product).
"""
import pytest
import torch

import gemm_oracle as go
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.knobs import KNOBS
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops import fc
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.nmse import StreamNMSE
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel

pytestmark = pytest.mark.gpu

D, F32, BF, F8 = torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn
NAN = float("nan")

# cfg -> (tile rows BM, tile columns BN, K steps in pairs) of the kernel's C[I, J]: 16 MF WM x 16 NJ WN of the Geo
# alias the launcher picks; pairs: KS = 2 (STEP_LOOP) or direct-A (ADIR) geometries
FWD = {0: (144, 128, False), 1: (192, 128, False), 2: (144, 128, True), 3: (192, 128, False), 4: (192, 128, False),
       5: (192, 128, True), 6: (192, 128, False), 7: (192, 128, False), 8: (144, 128, False), 9: (192, 128, False),
       10: (192, 128, False)}
WGRAD = {0: (128, 256, False), 1: (128, 256, False), 2: (128, 256, True), 3: (128, 256, False), 4: (128, 128, False),
         5: (256, 128, False), 6: (128, 256, False), 7: (128, 256, False)}    # I = N, J = K, reduction over M
DGRAD = {0: (144, 256, False), 1: (144, 128, False), 2: (144, 256, False), 3: (144, 256, True), 4: (288, 128, False),
         5: (144, 256, False), 6: (144, 256, False)}                           # I = M, J = K, reduction over N
KS = (64, 128, 192, 256, 320)
# (mode, variant, bias) of a sweep: both lattice forms, per-column scales, and the cancellation case
KINDS = (("lattice", "scaled", True), ("lattice", "scaled", False), ("real", "scaled", True), ("real", "cancel", False))


def bf(t, dev):
    return None if t is None else t.to(F32).to(BF).to(dev).contiguous()     # (exact: the operands are bf16 values)


def f8(t, dev):
    return t.to(F32).to(F8).to(dev).contiguous()                             # (exact: the operands are e4m3 values)


def nan(dev, *shape, dtype=BF):
    return torch.full(shape, NAN, device=dev, dtype=dtype)


def ff8(dev, *shape):
    return torch.full(shape, 0xFF, device=dev, dtype=torch.uint8).view(F8)


def scal(dev, *v):
    return torch.tensor(v, device=dev, dtype=F32)


class Check:
    """Collects the failures of one test's cases: exact on the lattice, max(err / bound) <= 1 on real data."""

    def __init__(self):
        self.fails, self.n = [], 0

    def cmp(self, what, case, mode, got, ref, bound=None, ref_exact=None):
        """lattice: got == ref_exact (default ref) bit for bit; real: |got - ref| <= bound everywhere."""
        self.n += 1
        got = got.detach().to(D).reshape(ref.shape)
        if mode == "lattice":
            msg = go.mismatch(f"{what} {case}", got, ref if ref_exact is None else ref_exact)
            if msg:
                self.fails.append(msg)
            return
        r = go.worst_ratio((got - ref).abs(), bound)
        print(f"ERRBOUND {what} {case} {r:.4f}")
        if not r <= 1.0:
            q = ((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).flatten()
            i = int(q.argmax())
            self.fails.append(f"{what} {case}: max err / bound = {r} at flat index {i}: got {float(got.flatten()[i])} "
                              f"ref {float(ref.flatten()[i])} bound {float(bound.flatten()[i])}")

    def gemm(self, what, case, g, got, f32=False):
        self.cmp(what, case, g.mode, got, g.exact, g.bound(f32), None if f32 else g.out_bf16())

    def true(self, cond, msg):
        self.n += 1
        if not cond:
            self.fails.append(msg)

    def done(self):
        torch.cuda.synchronize()
        assert self.n > 0 and not self.fails, "\n".join(self.fails)


def lattice_has_ties(g):
    assert g.mode != "lattice" or g.n_ties > 0, "no bf16 tie among the lattice sums"


# ================================================================================ 1. bf16 GEMMs, K sweep per cfg
@pytest.mark.parametrize("cfg", sorted(FWD))
def test_fwd_bf16(cuda, cfg):
    BM, BN, pairs = FWD[cfg]
    ck, M = Check(), 576
    for N, ks in ((256, KS), (128, (192, 256))):
        for K in ks:
            if pairs and (K // 64) % 2:
                continue
            for mode, variant, bias in KINDS:
                assert M % BM == 0 and N % BN == 0 and fc.gemm_fwd_ok(M, N, K, cfg), (M, N, K, cfg)
                g = go.gemm(mode, "bf16", M, N, K, 0, bias, variant, cuda)
                lattice_has_ties(g)
                Y = nan(cuda, M, N)
                fc.gemm_fwd(bf(g.P8, cuda), bf(g.Q8, cuda), bf(g.bias, cuda), out=Y, cfg=cfg)
                ck.gemm("fwd", f"cfg{cfg} N{N} K{K} {mode}/{variant}/bias{int(bias)}", g, Y)
    ck.done()


@pytest.mark.parametrize("cfg", sorted(WGRAD))
def test_wgrad_bf16(cuda, cfg):
    BM, BN, pairs = WGRAD[cfg]
    ck, N, K = Check(), 256, 256
    for M in KS:
        if pairs and (M // 64) % 2:
            continue
        for mode, variant in (("lattice", "scaled"), ("real", "scaled"), ("real", "cancel")):
            assert N % BM == 0 and K % BN == 0 and fc.gemm_wgrad_ok(M, N, K, cfg), (M, N, K, cfg)
            g = go.gemm(mode, "bf16", N, K, M, 1, False, variant, cuda)      # P = dY^T (N, M), Q = A^T (K, M)
            buf = nan(cuda, N, K + 64, dtype=F32)                            # ldw > K: the padding must stay NaN
            fc.gemm_wgrad(bf(g.P8.t(), cuda), bf(g.Q8.t(), cuda), out=buf[:, :K], cfg=cfg)
            case = f"cfg{cfg} M{M} {mode}/{variant}"
            ck.gemm("wgrad", case, g, buf[:, :K], f32=True)
            ck.true(bool(torch.isnan(buf[:, K:]).all()), f"wgrad {case}: wrote past column K of a strided output")
    ck.done()


@pytest.mark.parametrize("cfg", sorted(DGRAD))
def test_dgrad_bf16(cuda, cfg):
    BM, BN, pairs = DGRAD[cfg]
    ck, K = Check(), 256
    for M in (288, 576) if cfg == 4 else (288,):
        for N in KS:
            if pairs and (N // 64) % 2:
                continue
            for mode, variant in (("lattice", "scaled"), ("real", "scaled"), ("real", "cancel")):
                assert M % BM == 0 and K % BN == 0 and fc.gemm_dgrad_ok(M, N, K, cfg), (M, N, K, cfg)
                g = go.gemm(mode, "bf16", M, K, N, 2, False, variant, cuda)  # P = dY (M, N), Q = W^T (K, N)
                lattice_has_ties(g)
                dA = nan(cuda, M, K)
                fc.gemm_dgrad(bf(g.P8, cuda), bf(g.Q8.t(), cuda), out=dA, cfg=cfg)
                ck.gemm("dgrad", f"cfg{cfg} M{M} N{N} {mode}/{variant}", g, dA)
    ck.done()


# ================================================================================ 2. e4m3 GEMMs
F8KINDS = (("lattice", "scaled"), ("real", "scaled"), ("real", "cancel"))


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_fwd_f8(cuda, cfg):
    ck, M, N = Check(), 144, 128
    for K in (128, 256, 512):
        if cfg >= 1 and K % 256:        # (the MX-scaled MFMA takes K in steps of 256; the wrapper would run cfg 0)
            continue
        for mode, variant in F8KINDS:
            for bias in (True, False):
                g = go.gemm(mode, "e4m3", M, N, K, 3, bias, variant, cuda)
                lattice_has_ties(g)
                Y = nan(cuda, M, N)
                fc.gemm_fwd_f8(f8(g.P8, cuda), f8(g.Q8, cuda), scal(cuda, g.sP, g.sQ), bf(g.bias, cuda), out=Y, cfg=cfg)
                ck.gemm("fwd_f8", f"cfg{cfg} K{K} {mode}/{variant}/bias{int(bias)}", g, Y)
    ck.done()


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("cfg,I,J", [(1, 144, 128), (2, 128, 256)])
def test_nt_f8(cuda, cfg, I, J, f32):
    ck = Check()
    for K in (256, 512):
        for mode, variant in F8KINDS:
            g = go.gemm(mode, "e4m3", I, J, K, 4, False, variant, cuda)
            C = nan(cuda, I, J, dtype=F32 if f32 else BF)
            fc.gemm_nt_f8(f8(g.P8, cuda), f8(g.Q8, cuda), scal(cuda, g.sP), scal(cuda, g.sQ), out=C, cfg=cfg)
            ck.gemm("nt_f8", f"cfg{cfg} K{K} f32{int(f32)} {mode}/{variant}", g, C, f32=f32)
    ck.done()


def test_wgrad_f8(cuda):
    ck = Check()
    for M, N, K in ((256, 128, 256), (512, 256, 512)):
        for mode, variant in F8KINDS:
            g = go.gemm(mode, "e4m3", N, K, M, 5, False, variant, cuda)       # P = dY8^T (N, M), Q = A8^T (K, M)
            buf = nan(cuda, N, K + 64, dtype=F32)
            fc.gemm_wgrad_f8(f8(g.P8.t(), cuda), f8(g.Q8.t(), cuda), scal(cuda, g.sP), scal(cuda, g.sQ),
                             out=buf[:, :K])
            case = f"M{M} N{N} K{K} {mode}/{variant}"
            ck.gemm("wgrad_f8", case, g, buf[:, :K], f32=True)
            ck.true(bool(torch.isnan(buf[:, K:]).all()), f"wgrad_f8 {case}: wrote past column K")
    ck.done()


@pytest.mark.parametrize("cfg", [0, 1])
def test_dgrad_f8(cuda, cfg):
    ck = Check()
    for M, N, K in ((144, 256, 128), (288, 512, 256)):
        for mode, variant in F8KINDS:
            g = go.gemm(mode, "e4m3", M, K, N, 6, False, variant, cuda)       # P = dY8 (M, N), Q = W8^T (K, N)
            lattice_has_ties(g)
            dA = nan(cuda, M, K)
            fc.gemm_dgrad_f8(f8(g.P8, cuda), f8(g.Q8.t(), cuda), scal(cuda, g.sP), scal(cuda, g.sQ), out=dA, cfg=cfg)
            ck.gemm("dgrad_f8", f"cfg{cfg} M{M} N{N} K{K} {mode}/{variant}", g, dA)
    ck.done()


@pytest.mark.parametrize("cfg,K", [(0, 128), (0, 256), (1, 256), (2, 256)])
def test_e4m3_mfma_keeps_14_bits_below_the_largest_product(cuda, cfg, K):
    """The hardware property gemm_oracle.fma_term's ``align`` term rests on.  Row i of A8 is [448, -448, s, s, ...] and
    every row of W8 [448, 448, 1, 1, ...]: the two large products (2^17.6) cancel exactly and the exact result is
    (K - 2) s.  Products s >= 8 = 2^(17 - 14) must arrive exactly; a smaller s may lose whole addends to the
    alignment (measured: the 6 or 14 that share an 8-k block with a large product are dropped for every s <= 4, with
    the non-scaled MFMA and the MX-scaled one alike), but never more than s per product."""
    svals = [2.0 ** -9, 2.0 ** -6, 0.125, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0]
    s = torch.tensor(svals, dtype=F32).repeat(14)[:144]
    for k0, k1 in ((0, 1), (0, 64), (5, 77)):
        A = s[:, None].repeat(1, K)
        W = torch.ones(128, K)
        A[:, k0], A[:, k1], W[:, k0], W[:, k1] = 448.0, -448.0, 448.0, 448.0
        Y = nan(cuda, 144, 128)
        fc.gemm_fwd_f8(f8(A, cuda), f8(W, cuda), scal(cuda, 1.0, 1.0), None, out=Y, cfg=cfg)
        got, exact = Y.to(D).cpu(), ((K - 2) * s.to(D))[:, None].expand(144, 128)
        lost = (exact - got) / s.to(D)[:, None]            # addends lost (s 126 and s 254 are bf16 values)
        print(f"E4M3ALIGN cfg{cfg} K{K} large at k={k0},{k1}: addends lost per s = "
              f"{[round(float(lost[i, 0]), 2) for i in range(len(svals))]}")
        big = s >= 2.0 ** (17 - go.ALIGN_BITS)
        assert torch.equal(got[big], exact[big]), "a product within 14 bits of the largest one was not added exactly"
        assert bool((lost >= 0).all()) and bool((lost <= K - 2).all())


@pytest.mark.parametrize("R,C", [(64, 256), (192, 512)])
def test_transpose_u8(cuda, R, C):
    src = torch.randint(0, 256, (R, C), generator=torch.Generator().manual_seed(R), dtype=torch.uint8).to(cuda)
    dst = torch.full((C, R), 0xFF, device=cuda, dtype=torch.uint8)
    src[3, 5] = 0xFF     # (the prefill value occurs in the data too)
    fc.transpose_u8(src, out=dst)
    torch.cuda.synchronize()
    assert torch.equal(dst, src.t().contiguous())


# ================================================================================ 3. the shipped cfgs, flagship shape
FM, FN, FK = 2304, 2048, 4096     # the only shape whose grid takes the XCD-grouped branch of tile_of


def _flag(cuda, fmt, I, J, K, bias=False):
    g = go.Gemm("lattice", fmt, I, J, K, 7, bias, "scaled", cuda)             # (not cached: 300 MB of float64 each)
    assert go.bf16_ties(g.exact) > 0
    return g


def test_flagship_fwd_cfg8(cuda):
    assert fc.gemm_fwd_ok(FM, FN, FK, 8)
    g = _flag(cuda, "bf16", FM, FN, FK, True)
    Y = nan(cuda, FM, FN)
    fc.gemm_fwd(bf(g.P8, cuda), bf(g.Q8, cuda), bf(g.bias, cuda), out=Y, cfg=8)
    go.assert_equal("flagship fwd cfg 8", Y, g.out_bf16())


def test_flagship_wgrad_cfg7(cuda):
    assert fc.gemm_wgrad_ok(FM, FN, FK, 7)
    g = _flag(cuda, "bf16", FN, FK, FM)
    dW = nan(cuda, FN, FK, dtype=F32)
    fc.gemm_wgrad(bf(g.P8.t(), cuda), bf(g.Q8.t(), cuda), out=dW, cfg=7)
    go.assert_equal("flagship wgrad cfg 7", dW, g.out_f32())


def test_flagship_dgrad_cfg6(cuda):
    assert fc.gemm_dgrad_ok(FM, FN, FK, 6)
    g = _flag(cuda, "bf16", FM, FK, FN)
    dA = nan(cuda, FM, FK)
    fc.gemm_dgrad(bf(g.P8, cuda), bf(g.Q8.t(), cuda), out=dA, cfg=6)
    go.assert_equal("flagship dgrad cfg 6", dA, g.out_bf16())


def test_flagship_fwd_f8_cfg2(cuda):
    g = _flag(cuda, "e4m3", FM, FN, FK, True)
    Y = nan(cuda, FM, FN)
    fc.gemm_fwd_f8(f8(g.P8, cuda), f8(g.Q8, cuda), scal(cuda, g.sP, g.sQ), bf(g.bias, cuda), out=Y, cfg=2)
    go.assert_equal("flagship fwd_f8 cfg 2", Y, g.out_bf16())


def test_flagship_wgrad_f8(cuda):
    g = _flag(cuda, "e4m3", FN, FK, FM)
    dW = nan(cuda, FN, FK, dtype=F32)
    fc.gemm_wgrad_f8(f8(g.P8.t(), cuda), f8(g.Q8.t(), cuda), scal(cuda, g.sP), scal(cuda, g.sQ), out=dW)
    go.assert_equal("flagship wgrad_f8", dW, g.out_f32())


def test_flagship_dgrad_f8_cfg1(cuda):
    g = _flag(cuda, "e4m3", FM, FK, FN)
    dA = nan(cuda, FM, FK)
    fc.gemm_dgrad_f8(f8(g.P8, cuda), f8(g.Q8.t(), cuda), scal(cuda, g.sP), scal(cuda, g.sQ), out=dA, cfg=1)
    go.assert_equal("flagship dgrad_f8 cfg 1", dA, g.out_bf16())


# ================================================================================ 4. expert-routed forward
@pytest.mark.parametrize("cfg", [0, 8])
def test_routed_forward_equals_forward_on_gathered_rows(cuda, cfg):
    M, N, K, NE = 576, 256, 320, 3
    g = go.gemm("real", "bf16", M * NE, N, K, 8, True, "scaled", cuda)
    expert = torch.randint(0, NE, (M,), generator=torch.Generator().manual_seed(5)).to(cuda)
    A, W, b = bf(g.P8, cuda), bf(g.Q8, cuda), bf(g.bias, cuda)
    Y = nan(cuda, M, N)
    fc.gemm_fwd(A, W, b, out=Y, cfg=cfg, expert=expert, n_experts=NE)
    Yg = fc.gemm_fwd(go.route(A, expert, NE).contiguous(), W, b, out=nan(cuda, M, N), cfg=cfg)
    torch.cuda.synchronize()
    assert torch.equal(Y.view(torch.int16), Yg.view(torch.int16))
    ref = go.route(g.P, expert, NE) @ g.Q.t() + g.bias
    S = go.route(g.P, expert, NE).abs() @ g.Q.abs().t() + g.bias.abs()
    r = go.worst_ratio((Y.to(D) - ref).abs(), go.bf16_bound(ref, K, S))
    print(f"ERRBOUND routed cfg{cfg} {r:.4f}")
    assert r <= 1.0


def test_routed_forward_refused_on_the_direct_a_tile(cuda):
    M, N, K, NE = 576, 256, 256, 3
    A, W = torch.ones(M * NE, K, device=cuda, dtype=BF), torch.ones(N, K, device=cuda, dtype=BF)
    Y = nan(cuda, M, N)
    with pytest.raises(RuntimeError):
        fc.gemm_fwd(A, W, None, out=Y, cfg=5, expert=torch.zeros(M, device=cuda, dtype=torch.int64), n_experts=NE)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all())


# ================================================================================ 5. BN-reduction epilogue
BM_BN = 144
UB = [(1, 48), (2, 72), (3, 64), (3, 80), (4, 60)]   # aligned groups, straddles at several offsets, a full last tile
PART_SENTINEL = 12345.0


def _bnred(ck, cuda, what, run, mode, U, B, HW, N, fmt):
    """One (mode, shape): dA against the GEMM oracle, the partial rows against the oracle on the STORED dA, and which
    (u, tile) rows are written -- on a NaN-prefilled and on a sentinel-prefilled ``part``."""
    M, K = 3 * U * B, go.CPE * HW
    case = f"U{U} B{B} HW{HW} N{N} {mode}"
    g = go.gemm(mode, fmt, M, K, N, 9, False, "scaled", cuda)
    lattice_has_ties(g)
    z, rec = go.bn_z(mode, M, HW, U), go.bn_records(mode, U, B)
    st = go.records(rec, ("mean", "inv", "a", "b"), cuda)           # the other record columns hold the sentinel
    assert float(st[:, :, 4:].min()) > 0.99 * go.SENTINEL
    zb = bf(z, cuda)
    over = go.bn_overlap(U, B, M, BM_BN).to(cuda)
    outs = []
    for fill in (NAN, PART_SENTINEL):
        dA = nan(cuda, M, K)
        part = torch.full((U, M // BM_BN, 2, go.EC), fill, device=cuda, dtype=F32)
        run(g, dA, zb, st, part, B, U, HW)
        outs.append((dA, part))
    (dA, part), (dA2, part2) = outs
    ck.gemm(f"{what} dA", case, g, dA)
    written = ~torch.isnan(part)
    ck.true(bool(torch.equal(written, over[:, :, None, None].expand_as(written))),
            f"{what} {case}: partial rows written {written.all(3).all(2).tolist()} != rows that share a row "
            f"{over.tolist()}")
    kept = part2 == PART_SENTINEL
    ck.true(bool(torch.equal(kept, ~over[:, :, None, None].expand_as(kept))),
            f"{what} {case}: a sentinel-prefilled partial row that shares no row was overwritten, or one that does was not")
    ck.true(bool(torch.equal(dA.view(torch.int16), dA2.view(torch.int16))) and
            bool(torch.equal(torch.where(over[:, :, None, None], part, 0), torch.where(over[:, :, None, None], part2, 0))),
            f"{what} {case}: two runs differ")
    refs = go.bn_partials(dA, z.to(cuda), rec, U, B, HW)            # from the kernel's own stored dA
    if mode == "lattice":
        go.bn_check_exact(refs)
    got = torch.nan_to_num(part.to(D), nan=0.0).sum(1)              # summed over the tile axis (float64: exact)
    for k in range(2):
        ck.cmp(f"{what} part[{k}]", case, mode, got[:, k], refs[k], go.sum_bound(B * HW, refs[2 + k]))


@pytest.mark.parametrize("cfg", [0, 2, 5, 6])
def test_dgrad_bnred(cuda, cfg):
    ck, N = Check(), 128

    def run(g, dA, zb, st, part, B, U, HW):
        M, K = dA.shape
        assert M % DGRAD[cfg][0] == 0 and K % DGRAD[cfg][1] == 0 and fc.gemm_dgrad_ok(M, N, K, cfg)
        fc.gemm_dgrad_bnred(bf(g.P8, cuda), bf(g.Q8.t(), cuda), dA, cfg, zb, st, part, B, U, HW)

    for U, B in UB:
        for mode in ("lattice", "real"):
            _bnred(ck, cuda, f"dgrad_bnred cfg{cfg}", run, mode, U, B, 128, N, "bf16")
    if cfg == 6:
        for mode in ("lattice", "real"):
            _bnred(ck, cuda, "dgrad_bnred cfg6", run, mode, 3, 64, 256, N, "bf16")
    ck.done()


@pytest.mark.parametrize("cfg", [0, 1])
def test_dgrad_f8_bnred(cuda, cfg):
    ck, N = Check(), 256

    def run(g, dA, zb, st, part, B, U, HW):
        fc.gemm_dgrad_f8_bnred(f8(g.P8, cuda), f8(g.Q8.t(), cuda), scal(cuda, g.sP), scal(cuda, g.sQ), dA, cfg, zb, st,
                               part, B, U, HW)

    for U, B in ((2, 72), (3, 80)):
        for mode in ("lattice", "real"):
            _bnred(ck, cuda, f"dgrad_f8_bnred cfg{cfg}", run, mode, U, B, 128, N, "e4m3")
    ck.done()


# ================================================================================ 6. loss epilogue
def _loss(ck, cuda, what, mode, fmt, cfg, E, U, B, N, K, perf, round_y, f8_out=False):
    M, S = E * U * B, E * U
    case = f"cfg{cfg} E{E} U{U} B{B} K{K} perf{int(perf)} {mode}"
    g = go.gemm(mode, fmt, M, N, K, 10 + E, True, "scaled", cuda)
    L = go.Loss(g, E, U, B, 0, perf, round_y)
    if mode == "lattice":
        L.check_exact()
    nm = StreamNMSE(HDCEModel.row_stream(E, U, B, cuda), S, N)
    assert torch.equal(nm.row_stream.long(), L.stream)
    nm.rowoff = L.rowoff.to(cuda)
    if fmt == "bf16":
        tm = int(nat.fn(nat.hip_lib(), "qd_gemm_nmse_colsum_rows", [fc._i, fc._i])(cfg, E))
        A, W, deq = bf(g.P8, cuda), bf(g.Q8, cuda), None
    else:
        tm = fc.gemm_tile_m(0)
        A, W, deq = f8(g.P8, cuda), f8(g.Q8, cuda), scal(cuda, g.sP, g.sQ)
    # the buffers gemm_fused would allocate, NaN-prefilled
    dY0 = nan(cuda, M, N)
    nm._gz = ((tm, N), dY0, nan(cuda, M // 16 * (N // 128) * 2, dtype=F32), nan(cuda, M // tm, N, dtype=F32),
              nan(cuda, S, 2, dtype=F32))
    for t in (nm.ss, nm.loss, nm.skip):
        t.fill_(NAN)
    bg = nan(cuda, N, dtype=F32)
    out8 = None
    if f8_out:
        out8 = (ff8(cuda, M, N), ff8(cuda, N, M), scal(cuda, L.qs), torch.zeros(4096, device=cuda))
    dY = nm.gemm_fused(A, W, bf(g.bias, cuda), L.label.to(F32), L.perf.to(F32) if perf else None, bg, (E, U, B),
                       L.rowden.to(F32), loss_scale=L.loss_scale, cfg=cfg, deq=deq, f8_out=out8)
    assert dY is dY0
    ck.cmp(f"{what} dY", case, mode, dY, L.gf, L.dY_bound(), L.dY)
    ck.cmp(f"{what} bias_grad", case, mode, bg, L.bias_grad, L.bias_grad_bound())
    ck.cmp(f"{what} den", case, mode, nm.ss[:, 1], L.den, L.den_bound())
    ck.cmp(f"{what} loss", case, "real", nm.loss, L.loss, L.loss_bound())      # (never exact: always bounded)
    ck.true(float(nm.skip) == 0.0, f"{what} {case}: skip = {float(nm.skip)}")
    if f8_out:
        dY8, dYt8, _, am = out8
        ck.cmp(f"{what} dY8", case, mode, dY8.to(F32), L.x8(), L.dY8_bound(), L.dY8)
        ck.true(bool(torch.equal(dYt8.view(torch.uint8), dY8.view(torch.uint8).t())), f"{what} {case}: dYt8 != dY8^T")
        ck.cmp(f"{what} amax", case, mode, am.max(), L.amax, L.err_g.max())
        ck.true(int((dY8.to(F32).abs() == 448).sum()) > 0, f"{what} {case}: no dY8 entry saturates")


@pytest.mark.parametrize("cfg", [0, 1, 2, 6, 8, 10])
def test_loss_epilogue_bf16(cuda, cfg):
    ck = Check()
    ks = (64, 192, 256, 320) + ((1344, 1408) if cfg == 8 else ())
    for K in ks:
        if FWD[cfg][2] and (K // 64) % 2:
            continue
        for perf in (True, False):
            for mode in ("lattice", "real"):
                assert fc.gemm_fwd_ok(576, 256, K, cfg) and 576 % fc.gemm_tile_m(cfg) == 0
                _loss(ck, cuda, "loss", mode, "bf16", cfg, 3, 3, 64, 256, K, perf, round_y=cfg == 8)
    ck.done()


# E != 3: the per-row wave_sum paths and the column sums with a runtime chunk.  The launcher takes E when the tile
# rows are a multiple of 16 E (and of 4 E on cfg 8): E = 1 on the 144-row tiles (cfg 0, 8) and a 192-row one (cfg 1),
# E = 2 and E = 4 on 192-row tiles only
@pytest.mark.parametrize("cfg,E,U,B", [(0, 1, 6, 96), (8, 1, 6, 96), (1, 1, 6, 96), (1, 2, 3, 96), (10, 2, 3, 96),
                                       (1, 4, 3, 48), (6, 4, 3, 48)])
def test_loss_epilogue_bf16_other_expert_counts(cuda, cfg, E, U, B):
    ck, M = Check(), E * U * B
    bm = fc.gemm_tile_m(cfg)
    assert M == 576 and bm == FWD[cfg][0] and bm % (16 * E) == 0 and (bm // (B * E) + 2) * E <= 64 and B % 16 == 0
    for K in (192, 256):
        for mode in ("lattice", "real"):
            assert fc.gemm_fwd_ok(M, 256, K, cfg)
            _loss(ck, cuda, "loss", mode, "bf16", cfg, E, U, B, 256, K, True, round_y=cfg == 8)
    ck.done()


@pytest.mark.parametrize("producers", [True, False])
def test_loss_epilogue_f8(cuda, monkeypatch, producers):
    """K = 128 runs the non-scaled e4m3 MFMA tile, K = 256 the MX-scaled one (with producer waves when ``producers``).
    dY here is the one output that sees the accumulator at fp32 level (the real labels lie near y, |d| << |y|):
    against the plain fp32 bound (K + 2) EPS_F32 S it measured 1.7253 at K = 128 -- the e4m3 MFMA's alignment of
    its products, see gemm_oracle.fma_term -- and 0.77 with that term in the bound."""
    monkeypatch.setattr(KNOBS, "f8_producers", producers)
    ck = Check()
    for K in (128, 256):
        for mode in ("lattice", "real"):
            _loss(ck, cuda, f"loss_f8 producers{int(producers)}", mode, "e4m3", 0, 3, 3, 64, 256, K, True, False, True)
    ck.done()


# ================================================================================ 7. refusals
def test_refused_shapes_raise_and_leave_the_outputs_untouched(cuda):
    """One shape per entry point that its launcher must reject: the wrapper raises and the NaN-prefilled outputs are
    untouched (these calls return before any launch)."""
    one = lambda *s: torch.ones(s, device=cuda, dtype=BF)
    one8 = lambda *s: torch.ones(s, device=cuda, dtype=F32).to(F8)
    s1 = scal(cuda, 1.0)
    outs = []

    def refused(f, *out):
        with pytest.raises((RuntimeError, ValueError)):
            f()
        outs.extend(out)

    Y = nan(cuda, 100, 256)                                    # M not a tile multiple
    refused(lambda: fc.gemm_fwd(one(100, 256), one(256, 256), None, out=Y, cfg=0), Y)
    Y2 = nan(cuda, 576, 256)                                   # odd K / 64 on a STEP_LOOP (KS = 2) cfg
    refused(lambda: fc.gemm_fwd(one(576, 192), one(256, 192), None, out=Y2, cfg=2), Y2)
    Y5 = nan(cuda, 576, 256)                                   # ... and on the direct-A cfg
    refused(lambda: fc.gemm_fwd(one(576, 192), one(256, 192), None, out=Y5, cfg=5), Y5)
    dW = nan(cuda, 256, 256, dtype=F32)                        # odd M / 64 on the KS = 2 wgrad; N not a tile multiple
    refused(lambda: fc.gemm_wgrad(one(192, 256), one(192, 256), out=dW, cfg=2), dW)
    dW2 = nan(cuda, 64, 256, dtype=F32)
    refused(lambda: fc.gemm_wgrad(one(256, 64), one(256, 256), out=dW2, cfg=0), dW2)
    dA = nan(cuda, 100, 256)                                   # M not a tile multiple; odd N / 64 on the KS = 2 dgrad
    refused(lambda: fc.gemm_dgrad(one(100, 128), one(128, 256), out=dA, cfg=0), dA)
    dA3 = nan(cuda, 288, 256)
    refused(lambda: fc.gemm_dgrad(one(288, 192), one(192, 256), out=dA3, cfg=3), dA3)
    # BN epilogue: 3 B < 144 (a tile would span three groups)
    U, B = 3, 32
    dAb, part = nan(cuda, 288, 4096), nan(cuda, U, 2, 2, 96, dtype=F32)
    st = torch.zeros(U, 96, 8, device=cuda)
    for cfg in (0, 2, 5, 6):
        refused(lambda: fc.gemm_dgrad_bnred(one(288, 128), one(128, 4096), dAb, cfg, one(288, 4096), st, part, B, U, 128),
                dAb, part)
    part2 = nan(cuda, 2, 2, 2, 96, dtype=F32)                  # a cfg without the epilogue
    refused(lambda: fc.gemm_dgrad_bnred(one(288, 128), one(128, 4096), dAb, 1, one(288, 4096), st, part2, 48, 2, 128),
            dAb, part2)
    refused(lambda: fc.gemm_dgrad_f8_bnred(one8(288, 256), one8(256, 4096), s1, s1, dAb, 0, one(288, 4096), st, part, B, U,
                                           128), dAb, part)
    # e4m3 entries
    Y8 = nan(cuda, 100, 128)
    refused(lambda: fc.gemm_fwd_f8(one8(100, 256), one8(128, 256), scal(cuda, 1.0, 1.0), None, out=Y8, cfg=1), Y8)
    C8 = nan(cuda, 144, 128)
    refused(lambda: fc.gemm_nt_f8(one8(144, 128), one8(128, 128), s1, s1, out=C8, cfg=1), C8)      # K % 256
    dW8 = nan(cuda, 128, 256, dtype=F32)
    refused(lambda: fc.gemm_wgrad_f8(one8(128, 128), one8(128, 256), s1, s1, out=dW8), dW8)        # M % 256
    dA8 = nan(cuda, 144, 128)
    refused(lambda: fc.gemm_dgrad_f8(one8(144, 128), one8(128, 128), s1, s1, out=dA8, cfg=0), dA8)  # N % 256
    T8 = torch.full((256, 32), 0xFF, device=cuda, dtype=torch.uint8)
    refused(lambda: fc.transpose_u8(torch.zeros(32, 256, device=cuda, dtype=torch.uint8), out=T8))  # R % 64
    torch.cuda.synchronize()
    assert bool((T8 == 0xFF).all())
    for t in outs:
        assert bool(torch.isnan(t).all())


@pytest.mark.parametrize("E,U,B,cfg", [(5, 2, 96, 1), (2, 3, 96, 0), (3, 2, 24, 0)])
def test_loss_epilogue_refusals(cuda, E, U, B, cfg):
    """E = 5; E = 2 on a 144-row tile (not a multiple of 16 E); B not a multiple of 16: gemm_fused raises before any
    launch and leaves dY, the bias gradient and the loss untouched."""
    M, N, K, S = E * U * B, 256, 256, E * U
    nm = StreamNMSE(HDCEModel.row_stream(E, U, B, cuda), S, N)
    nm.rowoff = torch.arange(M, device=cuda, dtype=torch.int32)
    tm = int(nat.fn(nat.hip_lib(), "qd_gemm_nmse_colsum_rows", [fc._i, fc._i])(cfg, E))
    dY0 = nan(cuda, M, N)
    nm._gz = ((tm, N), dY0, nan(cuda, M // 16 * 2 * 2 + 2, dtype=F32), nan(cuda, M // tm + 1, N, dtype=F32),
              nan(cuda, S, 2, dtype=F32))
    nm.loss.fill_(NAN)
    bg = nan(cuda, N, dtype=F32)
    A = torch.ones(M, K, device=cuda, dtype=BF)
    with pytest.raises(RuntimeError):
        nm.gemm_fused(A, torch.ones(N, K, device=cuda, dtype=BF), None, torch.ones(M, N, device=cuda), None, bg, (E, U, B),
                      torch.ones(M, 2, device=cuda), cfg=cfg)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dY0, bg, nm.loss, *nm._gz[2:]))
