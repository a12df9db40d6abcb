"""Float64 oracle of the FC GEMM kernels (csrc/hip/gemm.hip): operand generators, references, exactness conditions
and the derived error bounds.  Pure torch, any device; a helper module, not a conftest.  The number formats, the
record layout, ``worst_ratio``, ``mismatch`` and ``sum_bound`` are tests/conv_oracle.py's.

Every GEMM is C[I, J] = sum_k P[i, k] Q[j, k] (+ bias[j]) -- the kernel template's own form:

  forward   Y  (M, N) = A W^T + b        P = A (M, K),      Q = W (N, K)         bf16 out
  wgrad     dW (N, K) = dY^T A           P = dY^T (N, M),   Q = A^T (K, M)       fp32 out
  dgrad     dA (M, K) = dY W             P = dY (M, N),     Q = W^T (K, N)       bf16 out
  e4m3      C = sP sQ P8 Q8^T (+ b)      the same with dequantisation scales     bf16 or fp32 out

Two kinds of operands, as in conv_oracle.  LATTICE: small integers (e4m3: integers of magnitude <= 16 and
power-of-two scales) such that sum_k |P[i, k]| |Q[j, k]| < 2^24 lattice units for every output: every partial sum
the kernel can form, in any order and any split over waves, is then an integer below 2^24 and exact in fp32, so the
accumulator IS the float64 sum and the stored output is its ONE rounding to the output format -- the kernel must
equal the reference bit for bit.  Every fourth row of Q is "loud" (dense integers up to 16), so the sums pass 256
and hit bf16 ties (257 -> 256, 259 -> 260): truncation and round-half-up both fail.  REAL: randn operands rounded
to the operand format, the rows of Q (the output's columns) scaled over 2^-6 .. 2^6 ("scaled") or P carrying a
common offset of 16 so that |ref| << S ("cancel"), checked element by element against ``f32_bound`` / ``bf16_bound``.
"""
from __future__ import annotations

import functools
import math

import torch

from conv_oracle import (D, EPS_BF16, EPS_F32, REC, SENTINEL, assert_equal, mismatch, records, round_bf16,  # noqa: F401
                         sum_bound, worst_ratio)

BK = 64               # K step of the kernels
E4M3_MAX = 448.0
EPS_E4M3 = 2.0 ** -4  # unit roundoff of e4m3 (4 significant bits)
F32 = torch.float32


# ------------------------------------------------------------------------------------------ number formats
def _exp(x: torch.Tensor) -> torch.Tensor:
    """frexp's exponent from the bits (|x| in [2^(e-1), 2^e); exact on any device)."""
    return ((x.to(D).view(torch.int64) >> 52) & 0x7FF) - 1022


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64, built from the bits (normal range)."""
    return ((e.to(torch.int64) + 1023) << 52).view(D)


def is_pow2(x: torch.Tensor) -> bool:
    b = x.to(D).view(torch.int64)
    return bool(((b & ((1 << 52) - 1)) == 0).all()) and bool((x > 0).all())


def round_e4m3(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest OCP e4m3 value (ties to even), ONE rounding, as float64: clamped to +-448 first (as
    common.h e4m3_pack4), 3 mantissa bits in the normal range (|x| >= 2^-6: spacing 2^(e-3) for |x| in [2^e, 2^(e+1))),
    spacing 2^-9 below it (the subnormals).  NaN stays NaN."""
    x = x.to(D).clamp(-E4M3_MAX, E4M3_MAX)
    step = _pow2(_exp(x).clamp_min(-5) - 4)      # |x| in [2^(e-1), 2^e): 4 significant bits
    return torch.round(x / step) * step          # (torch.round: halves to even; a power-of-two step: exact)


def is_e4m3(x: torch.Tensor) -> bool:
    return bool(torch.equal(round_e4m3(x), x.to(D)))


_LOW = (1 << 45) - 1   # the mantissa bits of a float64 below bf16's 7


def bf16_ties(x: torch.Tensor) -> int:
    """How many values lie exactly half way between two neighbouring bf16 values."""
    return int(((x.to(D).view(torch.int64) & _LOW) == (1 << 44)).sum())


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16 by truncation (a wrong store, for the mutation tests)."""
    return (x.to(D).view(torch.int64) & ~_LOW).view(D)


def flip_room(y: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    """Where a value within ``err`` of y can round to another bf16 value than y does (a rounding boundary -- the
    midpoint of two neighbours -- lies within err of y): the distance between the two, one bf16 ulp; else 0."""
    y = y.to(D)
    ulp = _pow2(_exp(y) - 8)
    t = y / ulp
    dist = ((t - torch.floor(t)) - 0.5).abs() * ulp
    return torch.where(dist <= err, ulp, torch.zeros_like(ulp))


# ------------------------------------------------------------------------------------------ derived bounds
ALIGN_BITS = 14   # an e4m3 MFMA keeps a product's bits down to 2^-14 of its largest neighbour's power of two


def fma_term(K: int, S: torch.Tensor, align=0.0) -> torch.Tensor:
    """``fma`` = (K + 2) EPS_F32 S (+ align): the fp32 accumulation of K exact products (bf16 x bf16 and e4m3 x e4m3
    products are exact in fp32) in ANY order and grouping is K - 1 roundings, each at most EPS_F32 times a partial
    sum of magnitude <= S = sum |p| |q| (first order); the epilogue adds at most three more on values <= S: the
    product of the two dequantisation scales, the accumulator times it, and the bias addition (S includes |bias|).

    ``align`` (e4m3 operands only, ``e4m3_align``): the e4m3 MFMAs -- v_mfma_f32_16x16x32_fp8_fp8 and the MX-scaled
    v_mfma_scale_f32_16x16x128_f8f6f4 alike -- do NOT add exact products in fp32.  Measured on the MI355X
    (tests/test_gemm_exact_gpu.py::test_e4m3_mfma_keeps_14_bits_below_the_largest_product): with products 448 x 448
    and -448 x 448 among the k of one instruction, products of magnitude <= 4 next to them are dropped whole and
    products >= 8 = 2^(17 - 14) arrive exactly, whatever the kernel's loop: the products of a block are aligned to
    the block's largest one, 2^E <= max |p q|, and truncated below 2^(E - 14).  So every product carries an error
    below 2^-14 max_k |p_k q_k| <= 2^-14 max_k |p_k| max_k |q_k|, K of them per output.  The bf16 MFMA shows no such
    term (its fp32 outputs reach 0.02 of (K + 2) EPS_F32 S)."""
    return (K + 2) * EPS_F32 * S + align


def e4m3_align(P: torch.Tensor, Q: torch.Tensor) -> torch.Tensor:
    """(I, J): K 2^-ALIGN_BITS max_k |P[i, k]| max_k |Q[j, k]| -- see fma_term."""
    return P.shape[1] * 2.0 ** -ALIGN_BITS * (P.abs().amax(1)[:, None] * Q.abs().amax(1)[None, :])


def f32_bound(K: int, S: torch.Tensor, align=0.0) -> torch.Tensor:
    """fp32 output: |err| <= fma."""
    return fma_term(K, S, align)


def bf16_bound(ref: torch.Tensor, K: int, S: torch.Tensor, align=0.0) -> torch.Tensor:
    """bf16 output: the fp32 value v is within fma of ref and the store is ONE rounding of v,
    |bf16(v) - ref| <= EPS_BF16 |v| + |v - ref| <= EPS_BF16 |ref| + (1 + EPS_BF16) fma."""
    return EPS_BF16 * ref.abs() + (1 + EPS_BF16) * fma_term(K, S, align)


def e4m3_bound(x: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    """e4m3 output of a value within ``err`` of x (x already scaled): the clamp to +-448 is a contraction, then one
    rounding: half a spacing, EPS_E4M3 |x| in the normal range and 2^-10 below 2^-6."""
    xc = x.abs().clamp_max(E4M3_MAX)
    return torch.maximum(EPS_E4M3 * xc, torch.full_like(xc, 2.0 ** -10)) + (1 + EPS_E4M3) * err


# ------------------------------------------------------------------------------------------ GEMM operands
def _gen(seed: int, *dims: int) -> torch.Generator:
    s = seed
    for d in dims:
        s = (s * 1000003 + d) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(D)


class Gemm:
    """Operands and reference of one C = sP sQ P Q^T (+ bias).  ``fmt``: "bf16" or "e4m3".  P (I, K), Q (J, K): the
    dequantised values; P8 / Q8: the values before the scales (what the e4m3 tensors hold; bf16: P, Q themselves).
    exact: the float64 result; S: the same product of absolute values (+ |bias|)."""

    def __init__(self, mode: str, fmt: str, I: int, J: int, K: int, seed: int = 0, bias: bool = False,
                 variant: str = "scaled", device="cpu"):
        assert mode in ("lattice", "real") and fmt in ("bf16", "e4m3") and variant in ("scaled", "cancel")
        self.mode, self.fmt, self.I, self.J, self.K = mode, fmt, I, J, K
        g = _gen(seed, I, J, K, len(mode), len(fmt), len(variant))
        loud = (torch.arange(J) % 4 == 1)[:, None]
        if mode == "lattice":
            P = _ints(g, -3, 3, I, K) if fmt == "bf16" else _ints(g, -4, 4, I, K)
            quiet = _ints(g, -2, 2, J, K) * (torch.rand(J, K, generator=g) < 0.5)
            Q = torch.where(loud, _ints(g, -16, 16, J, K), quiet)
            self.sP, self.sQ = (1.0, 1.0) if fmt == "bf16" else (0.25, 2.0)
            # integer biases that are bf16 values: small ones, and even ones around +-256 and 384 (they carry the
            # quiet columns' sums to the bf16 ties too)
            off = torch.tensor([0., 256., -256., 384.], dtype=D)[torch.randint(0, 4, (J,), generator=g)]
            small = _ints(g, -9, 9, J)
            b = torch.where(off == 0, small, 2 * small) + off
        else:
            P = torch.randn(I, K, generator=g).to(D)
            Q = torch.randn(J, K, generator=g).to(D) * K ** -0.5
            if variant == "scaled":   # the output's columns over 2^-6 .. 2^6
                Q = Q * torch.ldexp(torch.ones(J, 1, dtype=D), torch.randint(-6, 7, (J, 1), generator=g))
            else:
                P = P + 16.0
            if fmt == "bf16":
                P, Q = round_bf16(P), round_bf16(Q)
                self.sP, self.sQ = 1.0, 1.0
            else:   # per-tensor scales (fp32 values) that put the largest element at 448, as the fp8 estimator's
                self.sP = float(torch.tensor(float(P.abs().max()) / E4M3_MAX, dtype=F32))
                self.sQ = float(torch.tensor(float(Q.abs().max()) / E4M3_MAX, dtype=F32))
                P, Q = round_e4m3(P / self.sP), round_e4m3(Q / self.sQ)
            b = round_bf16(torch.randn(J, generator=g).to(D))
        self.P8, self.Q8 = P.to(device), Q.to(device)
        self.P, self.Q = self.P8 * self.sP, self.Q8 * self.sQ
        self.bias = b.to(device) if bias else None
        self.exact = self.P @ self.Q.t()
        self.S = self.P.abs() @ self.Q.abs().t()
        if bias:
            self.exact = self.exact + self.bias
            self.S = self.S + self.bias.abs()
        # (the lattice's non-zero products lie in 1 .. 64: nothing is truncated there)
        self.align = e4m3_align(self.P, self.Q) if fmt == "e4m3" and mode == "real" else 0.0
        if mode == "lattice":
            self.check_exact()

    def fma(self) -> torch.Tensor:
        return fma_term(self.K, self.S, self.align)

    def check_exact(self) -> None:
        """The lattice condition: integer operands representable in the format, power-of-two scales, and
        sum |addend| < 2^24 lattice units for every output (the unit is sP sQ; an integer bias joins the sum)."""
        integer = lambda t: bool(torch.equal(t, t.round()))
        assert integer(self.P8) and integer(self.Q8)
        if self.fmt == "bf16":
            assert torch.equal(round_bf16(self.P8), self.P8) and torch.equal(round_bf16(self.Q8), self.Q8)
        else:
            assert is_e4m3(self.P8) and is_e4m3(self.Q8) and float(max(self.P8.abs().max(), self.Q8.abs().max())) <= 16
        unit = self.sP * self.sQ
        assert unit == 2.0 ** round(torch.log2(torch.tensor(unit)).item())
        if self.bias is not None:
            assert integer(self.bias) and torch.equal(round_bf16(self.bias), self.bias)
        assert float(self.S.max()) / min(unit, 1.0) < 2 ** 24, float(self.S.max())

    # ---- what the kernel must store
    def out_f32(self) -> torch.Tensor:
        return self.exact

    def out_bf16(self) -> torch.Tensor:
        return round_bf16(self.exact)

    def bound(self, f32: bool) -> torch.Tensor:
        return f32_bound(self.K, self.S, self.align) if f32 else bf16_bound(self.exact, self.K, self.S, self.align)


@functools.lru_cache(maxsize=None)
def gemm(mode, fmt, I, J, K, seed=0, bias=False, variant="scaled", device="cpu") -> Gemm:
    g = Gemm(mode, fmt, I, J, K, seed, bias, variant, device)
    if mode == "lattice":
        g.n_ties = bf16_ties(g.exact)   # (a case whose output is bf16 asserts that it has some)
    return g


def route(A: torch.Tensor, expert: torch.Tensor, n_experts: int) -> torch.Tensor:
    """Expert-routed rows: row i of the product uses A[i * n_experts + expert[i]]."""
    i = torch.arange(expert.numel(), device=A.device)
    return A[i * n_experts + expert.to(A.device).long()]


# ------------------------------------------------------------------------------------------ BN partials
NE, CPE, EC = 3, 32, 96   # experts, channels per expert, channels


def bn_records(mode: str, U: int, seed: int = 0) -> dict:
    """(U, 96) records mean, inv, a, b of the BN reduction epilogue.  Lattice: integer mean, power-of-two inv, a of
    both signs and b = integer + 0.5, so a z + b is never 0 for integer z -- except in channels 5 and 40, whose b is
    an integer: there a z + b == 0 occurs and the gate (strictly > 0) must be closed."""
    g = _gen(seed, U, 17)
    if mode == "lattice":
        pick = lambda vals: torch.tensor(vals, dtype=D)[torch.randint(0, len(vals), (U, EC), generator=g)]
        b = _ints(g, -3, 2, U, EC) + 0.5
        b[:, 5] += 0.5
        b[:, 40] -= 0.5
        return dict(mean=_ints(g, -1, 1, U, EC), inv=pick([0.5, 1.0, 2.0]), a=pick([1., 2., -1., -2.]), b=b)
    f32 = lambda t: t.to(F32).to(D)
    un = lambda lo, hi: lo + (hi - lo) * torch.rand(U, EC, generator=g)
    sg = torch.randint(0, 2, (U, EC), generator=g).to(F32) * 2 - 1
    return dict(mean=f32(0.3 * torch.randn(U, EC, generator=g)), inv=f32(un(0.5, 2.0)), a=f32(sg * un(0.5, 1.5)),
                b=f32(un(-0.5, 0.5)))


def bn_z(mode: str, M: int, HW: int, seed: int = 0) -> torch.Tensor:
    """The layer's pre-BN output in dA's layout: (M, 32 HW), row (u B + b) 3 + e, column c HW + p."""
    g = _gen(seed, M, HW, 23)
    return _ints(g, -4, 4, M, CPE * HW) if mode == "lattice" else round_bf16(torch.randn(M, CPE * HW, generator=g).to(D))


def bn_partials(dA: torch.Tensor, z: torch.Tensor, rec: dict, U: int, B: int, HW: int, gate_ge: bool = False):
    """(sum g, sum g xhat, sum |g|, sum |g xhat|), each (U, 96), of g = dA [a z + b > 0] and
    xhat = (z - mean) * inv evaluated in fp32 as common.h bn_xhat (one rounding per operation), from a STORED dA
    (M, 32 HW).  The gate in float64: a z + b of an fp32 a, b and a bf16 z has the sign of its fp32 fma."""
    dev = dA.device
    x = lambda t: t.to(D).reshape(U, B, NE, CPE, HW)
    per = lambda k: rec[k].to(dev).to(D).reshape(U, 1, NE, CPE, 1)   # channel e * 32 + c
    zz = x(z)
    v = per("a") * zz + per("b")
    gate = (v >= 0) if gate_ge else (v > 0)
    g = torch.where(gate, x(dA), torch.zeros((), dtype=D, device=dev))
    xhat = ((zz.to(F32) - per("mean").to(F32)) * per("inv").to(F32)).to(D)
    gx = g * xhat
    s = lambda t: t.sum(dim=(1, 4)).reshape(U, EC)
    return s(g), s(gx), s(g.abs()), s(gx.abs())


def bn_overlap(U: int, B: int, M: int, BM: int = 144) -> torch.Tensor:
    """(U, M / BM) bool: the (group, tile) pairs that share a row -- the partial rows the epilogue writes."""
    lo = torch.arange(M // BM) * BM
    u = torch.arange(U)[:, None] * (3 * B)
    return (lo[None, :] < u + 3 * B) & (lo[None, :] + BM > u)


def bn_check_exact(parts) -> None:
    """The lattice condition of the partials: sum |addend| < 2^24 units of 1/4 (xhat is a multiple of 1/2)."""
    for p in parts[2:]:
        assert float(p.max()) * 4 < 2 ** 24, float(p.max())


# ------------------------------------------------------------------------------------------ loss epilogue
class Loss:
    """The HDCE loss epilogue on one forward (see gemm.hip EPI_NMSE).  Rows r = (u B + b) E + e, stream s = e U + u.

      y      = acc + bias, rounded to bf16 when ``round_y`` (the bf16 cfg-8 tile, whose producer waves run the row
               pass of the plain forward + one-pass NMSE kernel pair: nmse_rows_prefetched; the compute waves' row
               pass uses the fp32 value)
      d      = y - label[rowoff[r]],  coef_s = loss_scale 2 / (S den_s),  den_s = sum_b rowden[r, 0]
      dY     = bf16(coef d);  bias gradient = sum_r coef d;  loss = mean_s (sum d^2 / den_s)  (and against perf)
      dY8    = e4m3(coef d qs);  amax = max |coef d|.  qs None: chosen so that the largest entries pass 448 and
               saturate (a power of two on the lattice, 1.5 x 448 / amax as an fp32 value on real data)

    Lattice: integer labels, dyadic rowden rows whose stream sums are powers of two, loss_scale = S 2^j: every
    coefficient is a power of two and everything but the loss pair is exact."""

    def __init__(self, g: Gemm, E: int, U: int, B: int, seed: int = 0, perf: bool = True, round_y: bool = False,
                 qs: float = None):
        M, N = g.I, g.J
        assert M == E * U * B and g.bias is not None
        self.g, self.E, self.U, self.B, self.M, self.N, self.Sn = g, E, U, B, M, N, E * U
        self.round_y, self.qs, dev = round_y, qs, g.exact.device
        gen = _gen(seed, M, N, E, 31)
        rows = M + 5                                                    # the label store, read through rowoff
        self.rowoff = torch.randperm(rows, generator=gen)[:M].to(torch.int32)
        r = torch.arange(M)
        self.stream = ((r % E) * U + r // (B * E)).to(dev)              # s = e U + u
        yex = g.exact.cpu()
        if g.mode == "lattice":
            lab = _ints(gen, -3, 3, rows, N)
            per = _ints(gen, -3, 3, rows, N)
            ks, kp = torch.randint(0, 3, (self.Sn,), generator=gen), torch.randint(0, 3, (self.Sn,), generator=gen)
            # a stream's rows b >= 1 alternate 1 / 512 and 3 / 512 and row 0 takes the rest of 1: dyadic rows whose
            # sum is 1 in any order (every partial sum is a multiple of 2^-9 below 2), times the stream's 2^k
            b = (r // E) % B
            w = torch.where(b % 2 == 0, 1.0, 3.0).to(D) / 512
            w = torch.where(b == 0, 1.0 - (3 * (B // 2) + (B - 1) // 2) / 512, w)
            st = self.stream.cpu()
            rowden = torch.stack([w * torch.ldexp(torch.ones(M, dtype=D), ks[st]),
                                  w * torch.ldexp(torch.ones(M, dtype=D), kp[st] + 1)], 1)
            self.loss_scale = float(self.Sn) * 0.25
        else:
            f32 = lambda t: t.to(F32).to(D)
            # labels near the prediction (|d| << |y|, a trained estimator's regime: the rounding of y then shows)
            lab = f32(torch.randn(rows, N, generator=gen).to(D))
            per = f32(torch.randn(rows, N, generator=gen).to(D))
            ro = self.rowoff.long()
            lab[ro] = f32(yex + 0.05 * yex.abs().mean(0, keepdim=True) * torch.randn(M, N, generator=gen).to(D))
            per[ro] = f32(lab[ro] + 0.02 * yex.abs().mean(0, keepdim=True) * torch.randn(M, N, generator=gen).to(D))
            rowden = torch.stack([f32(lab[ro].pow(2).sum(1)), f32(per[ro].pow(2).sum(1))], 1)
            self.loss_scale = 1.0
        self.label, self.perf, self.rowden = lab.to(dev), (per.to(dev) if perf else None), rowden.to(dev)
        self.has_perf = perf
        self._ref()

    def _ref(self) -> None:
        g, dev, Sn = self.g, self.g.exact.device, self.Sn
        ssum = lambda v: torch.zeros(Sn, dtype=D, device=dev).index_add_(0, self.stream, v)
        fma = g.fma()
        y = g.exact
        # the error of the kernel's y against this one: fma, plus a bf16 ulp where the rounding can flip
        self.err_y = fma
        if self.round_y:
            self.err_y = fma + flip_room(y, fma)
            y = round_bf16(y)
        self.y = y
        ro = self.rowoff.to(dev).long()
        self.den = ssum(self.rowden[:, 0])
        self.denp = ssum(self.rowden[:, 1])
        self.coef = (self.loss_scale * 2.0 / (Sn * self.den))[self.stream][:, None]
        self.d = y - self.label[ro]
        self.gf = self.coef * self.d                        # the fp32 gradient value
        self.dY = round_bf16(self.gf)
        # d carries err_y and its own subtraction's rounding; coef a division and two products (3 EPS_F32 relative)
        self.err_g = self.coef * self.err_y + 5 * EPS_F32 * self.gf.abs()
        self.bias_grad = self.gf.sum(0)
        self.bias_grad_abs = self.gf.abs().sum(0)
        self.num = ssum((self.d ** 2).sum(1))
        dp = y - self.perf[ro] if self.has_perf else torch.zeros_like(y)
        self.nump = ssum((dp ** 2).sum(1))
        # error of a stream's numerator: d^2 moves by (2 |d| + err) err per element, then an fp32 sum of B N squares
        e2 = lambda dd: ssum((((2 * dd.abs() + self.err_y) * self.err_y) + 2 * EPS_F32 * dd ** 2).sum(1))
        n = self.B * self.N
        self.num_err = e2(self.d) + sum_bound(n, self.num)
        self.nump_err = e2(dp) + sum_bound(n, self.nump)
        self.loss = torch.stack([(self.num / self.den).mean(),
                                 (self.nump / self.denp).mean() if self.has_perf else torch.zeros((), dtype=D, device=dev)])
        self.amax = self.gf.abs().max()
        if self.qs is None:
            r = E4M3_MAX / float(self.amax)
            self.qs = 2.0 ** (math.ceil(math.log2(r)) + 1) if g.mode == "lattice" else float(torch.tensor(1.5 * r, dtype=F32))
        self.dY8 = round_e4m3(self.gf * self.qs)

    # ---- bounds
    def dY_bound(self) -> torch.Tensor:
        """dY = bf16 of an fp32 value within err_g of coef d: EPS_BF16 |ref| + (1 + EPS_BF16) err_g."""
        return EPS_BF16 * self.gf.abs() + (1 + EPS_BF16) * self.err_g

    def x8(self) -> torch.Tensor:
        """What dY8 quantises, clamped as the kernel clamps it: the reference of the bounded dY8 comparison."""
        return (self.gf * self.qs).clamp(-E4M3_MAX, E4M3_MAX)

    def dY8_bound(self) -> torch.Tensor:
        """dY8 = e4m3 of (coef d) qs formed in fp32: one more product rounding on top of err_g."""
        x = self.gf * self.qs
        return e4m3_bound(x, abs(self.qs) * self.err_g + EPS_F32 * x.abs())

    def bias_grad_bound(self) -> torch.Tensor:
        """The bias gradient sums the fp32 gradient values (not the stored bf16 dY) over the M rows in fp32:
        sum_r err_g plus sum_bound(M, sum |coef d|)."""
        return self.err_g.sum(0) + sum_bound(self.M, self.bias_grad_abs)

    def loss_bound(self) -> torch.Tensor:
        """loss = (1 / S) sum_s num_s / den_s: each numerator within num_err (the propagated error of y and the fp32
        summation of its B N squares), one division each and the mean's S additions and division:
        (1 / S) sum_s num_err_s / den_s + (S + 3) EPS_F32 (1 / S) sum_s num_s / den_s.  den_s is the kernel's own
        fp32 sum of the rowden rows the test hands it (B EPS_F32 relative)."""
        out = []
        for num, err, den in ((self.num, self.num_err, self.den), (self.nump, self.nump_err, self.denp)):
            out.append((err / den).mean() + (self.Sn + 3 + self.B) * EPS_F32 * (num / den).mean())
        return torch.stack(out)

    def den_bound(self) -> torch.Tensor:
        return sum_bound(self.B, self.den)

    def check_exact(self) -> None:
        assert self.g.mode == "lattice"
        c = self.coef.flatten()
        assert is_pow2(c) and is_pow2(self.den) and bool(torch.equal(self.rowden.to(F32).to(D), self.rowden))
        assert bool(torch.equal(self.rowden * 2 ** 12, (self.rowden * 2 ** 12).round())) and float(self.rowden.min()) > 0
        cmin = float(c.min())
        assert float(self.bias_grad_abs.max()) / cmin < 2 ** 24
        assert float(self.d.abs().max()) < 2 ** 24 and bool(torch.equal(self.d * 8, (self.d * 8).round()))
