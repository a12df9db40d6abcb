"""Float64 oracle of the HDCE conv / BatchNorm / ReLU kernels (csrc/hip/conv.hip): data generators, references,
exactness conditions and the derived error bounds.  Pure torch, any device; a helper module, not a conftest.

Everything is for ``E`` groups of 32 channels on (N, E*C, 16, W) tensors with N = U groups x B samples; layer 1
has C = 2 input channels.  A BN record of a (group u, channel) is (mean, inv, a, b, c1, c2, c3):

  forward    h = bf16(relu(a * z_prev + b))            (layer 1: h = bf16(x1))
             z = conv3x3(h, bf16(w), padding 1, groups E), stored as bf16
             statistics: per (u, channel) sum z and sum z^2 of the STORED z
  backward   gate = a * z + b > 0 (float64: an fp32 x bf16 product plus an fp32 value, so its sign is the fma's)
             g = dh * gate, xhat = (z - mean) * inv, dz = (c1 * g - c2) - c3 * xhat -- one fp32 rounding per
             operation, as common.h's bn_xhat / bn_dz -- then dz rounded to bf16
             dx = conv_transpose(dz, w), dW = sum_n dz (x) h
             the previous layer's partials: sum g' and sum g' * xhat', g' = dx_stored * gate'
  S = conv(|h|, |w|), S_dx, S_dW: the sums of absolute products, the scale of the error bounds.

Two kinds of data: a small-integer LATTICE on which every intermediate of the kernels is exact in its number
format (the kernels must then equal this reference bit for bit, whatever their summation order), and REAL
randn-scaled data checked element by element against the bounds derived at ``fwd_bound`` .. ``sum_bound``.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

H = 16
CO = 32
NST = 8
E = 3
D = torch.float64
SENTINEL = 1e30       # fills the record columns a kernel must not read
EPS_BF16 = 2.0 ** -8  # unit roundoff of bf16 (8 significant bits, round to nearest even)
EPS_F32 = 2.0 ** -24  # unit roundoff of fp32
REC = ("mean", "inv", "a", "b", "c1", "c2", "c3")


# ------------------------------------------------------------------------------------------ number formats
def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 (ties to even), ONE rounding, as float64 (normal range; NaN stays NaN).  Integer
    arithmetic on the bits -- the 45 low mantissa bits rounded away, half to even -- so it is exact on any device
    (frexp / ldexp on the GPU gave 1159.9999999999998 for 1160)."""
    x = x.to(D)
    b = x.view(torch.int64)
    r = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    return torch.where(torch.isnan(x), x, r.view(D))


def is_bf16(x: torch.Tensor) -> bool:
    return bool(torch.equal(round_bf16(x), x.to(D)))


def is_f32(x: torch.Tensor) -> bool:
    return bool(torch.equal(x.to(torch.float32).to(D), x.to(D)))


# ------------------------------------------------------------------------------------------ the operation
def per_n(v: torch.Tensor, B: int) -> torch.Tensor:
    """(U, EC) per-(group, channel) values -> (N, EC, 1, 1)."""
    return v.repeat_interleave(B, dim=0)[:, :, None, None]


def group_sums(x: torch.Tensor, U: int) -> torch.Tensor:
    """(N, EC, H, W) -> (U, EC) sums over a group's samples and positions."""
    return x.reshape(U, x.shape[0] // U, x.shape[1], -1).sum(dim=(1, 3))


def bn_relu(z_prev: torch.Tensor, a: torch.Tensor, b: torch.Tensor, B: int) -> torch.Tensor:
    """h = relu(a z_prev + b) rounded once to bf16 (float64 in and out; NaN propagates as torch.relu does)."""
    return round_bf16(torch.relu(per_n(a, B) * z_prev + per_n(b, B)))


def h_flip_room(z_prev: torch.Tensor, a: torch.Tensor, b: torch.Tensor, B: int) -> torch.Tensor:
    """Where the fp32 evaluation of relu(a z_prev + b) can round to another bf16 value than the float64 one: the
    distance to it (one bf16 ulp; at the ReLU's kink the fp32 value itself), else 0.  The fp32 value -- an fma, or
    a rounded product and a sum -- is within err = 2^-23 (|a z| + |b|) of the exact y; the two roundings differ
    only if a bf16 rounding boundary (the midpoint of two neighbours) or zero lies within err of y."""
    az, bb = per_n(a, B) * z_prev, per_n(b, B)
    y = az + bb
    err = 2 * EPS_F32 * (az.abs() + bb.abs())
    _, e = torch.frexp(y)
    ulp = torch.ldexp(torch.ones_like(y), e - 8)
    t = y / ulp
    dist = ((t - torch.floor(t)) - 0.5).abs() * ulp
    room = torch.where((dist <= err) & (y > -err), ulp, torch.zeros_like(y))
    return torch.where(y.abs() <= err, torch.maximum(room, 2 * err), room)


def conv(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return F.conv2d(h, w, padding=1, groups=h.shape[1] // w.shape[1])


def conv_grads(h: torch.Tensor, w: torch.Tensor, dz: torch.Tensor):
    """(dx, dW) of z = conv(h, w) for the upstream gradient dz."""
    h = h.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(conv(h, w), (h, w), dz)
    return dx.detach(), dw.detach()


def bn_backward(dh: torch.Tensor, z: torch.Tensor, rec: dict, B: int, dt: torch.dtype = torch.float32):
    """(g, xhat, dz) of the BN / ReLU backward.  ``dt`` = float32 mirrors common.h rounding for rounding (eager torch
    rounds once per elementwise operation); float64 is the operation itself.  dz is NOT yet rounded to bf16."""
    p = {k: per_n(rec[k], B) for k in REC}
    gate = (p["a"] * z + p["b"]) > 0                      # float64
    g = torch.where(gate, dh, torch.zeros_like(dh))
    xhat = (z.to(dt) - p["mean"].to(dt)) * p["inv"].to(dt)
    dz = (p["c1"].to(dt) * g.to(dt) - p["c2"].to(dt)) - p["c3"].to(dt) * xhat
    return g, xhat.to(D), dz.to(D)


def bn_partials(g: torch.Tensor, xhat: torch.Tensor, U: int):
    """sum g, sum g * xhat per (u, channel), and the sums of absolute addends (their error scale)."""
    gx = g * xhat
    return group_sums(g, U), group_sums(gx, U), group_sums(g.abs(), U), group_sums(gx.abs(), U)


def records(rec: dict, cols, device=None) -> torch.Tensor:
    """(U, EC, NST) fp32 record tensor with the named columns set and the sentinel everywhere else."""
    U, EC = rec["a"].shape
    out = torch.full((U, EC, NST), SENTINEL, dtype=torch.float32)
    for k in cols:
        out[:, :, REC.index(k)] = rec[k].to(torch.float32)
    return out.to(device) if device is not None else out


# ------------------------------------------------------------------------------------------ derived bounds
def fwd_bound(ref: torch.Tensor, S: torch.Tensor) -> torch.Tensor:
    """Forward z: |z - ref| <= 2^-8 (|ref| + S).  The stored z is one bf16 rounding of the fp32 accumulator,
    EPS_BF16 * |ref|.  A staged h is relu(a z + b) evaluated in fp32 and then rounded to bf16, the reference's in
    float64; where the fp32 value (within 2^-23 of the exact one) straddles a bf16 rounding boundary the two land
    on neighbouring bf16 values.  The S term charges EVERY staged h with such a flip at 2^-8 |h| (it happens to a
    few in 10^5 of them), which leaves room for the fp32 accumulation of the 9 * 32 = 288 products,
    288 * EPS_F32 * S = 2^-15.8 S."""
    return EPS_BF16 * (ref.abs() + S)


def dgrad_bound(ref: torch.Tensor, S_dx: torch.Tensor) -> torch.Tensor:
    """Data gradient.  The staged dz is bit-exact (bn_backward mirrors the kernels' roundings), so what is left is
    the output's bf16 rounding, EPS_BF16 * |ref|, and the fp32 accumulation of 288 products,
    288 * EPS_F32 * S_dx < 2^-14 * S_dx."""
    return EPS_BF16 * ref.abs() + 2.0 ** -14 * S_dx


def sum_bound(n: int, S: torch.Tensor) -> torch.Tensor:
    """fp32 sums of n addends in ANY order: |fl(sum) - sum| <= (n - 1) EPS_F32 * sum |x_i| to first order, and the
    rounding of each addend (a product formed in fp32, or fused) is one more EPS_F32 * sum |x_i|."""
    return n * EPS_F32 * S


def ulp_bound(ref: torch.Tensor, floor: torch.Tensor) -> torch.Tensor:
    """A bf16 value computed in fp32 against the same value computed in float64: neighbouring bf16 values at most,
    one ulp <= 2^-7 |ref|; ``floor`` = the fp32 evaluation's own absolute error (matters where ref is ~0)."""
    return 2.0 ** -7 * ref.abs() + floor


def worst_ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound over all elements (inf where the bound is zero and the error is not; nan if err has NaN)."""
    err, bound = err.to(D), bound.to(D)
    if bool(torch.isnan(err).any()):
        return float("nan")
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------ mismatch report
def mismatch(name: str, got: torch.Tensor, ref: torch.Tensor, limit: int = 6):
    """None when ``got`` equals ``ref`` exactly (NaN == NaN); else a message with the count and the first
    (n, e, channel, row, col) indices, split into border and interior positions."""
    got, ref = got.detach().to(D).cpu(), ref.detach().to(D).cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad = ~((got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    lines = [f"{name}: {idx.shape[0]} of {bad.numel()} elements differ"]
    if got.dim() == 4:
        hh, ww = got.shape[2], got.shape[3]
        border = (idx[:, 2] == 0) | (idx[:, 2] == hh - 1) | (idx[:, 3] == 0) | (idx[:, 3] == ww - 1)
        for label, sel in (("border", idx[border]), ("interior", idx[~border])):
            lines.append(f"  {label}: {sel.shape[0]}")
            for n, ch, r, c in sel[:limit].tolist():
                cpe = got.shape[1] // E
                lines.append(f"    (n={n}, e={ch // cpe}, c={ch % cpe}, row={r}, col={c}): got {float(got[n, ch, r, c])}"
                             f" ref {float(ref[n, ch, r, c])}")
    else:
        for ix in idx[:limit].tolist():
            lines.append(f"    {tuple(ix)}: got {float(got[tuple(ix)])} ref {float(ref[tuple(ix)])}")
    return "\n".join(lines)


def assert_equal(name: str, got: torch.Tensor, ref: torch.Tensor) -> None:
    msg = mismatch(name, got, ref)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------ data
class Case:
    """The operands of one (mode, U, B, W, seed) and their references (computed once, on the CPU, and cached).

    x1 (N, E*2, H, W): layer 1's input.  z_prev / z (N, EC, H, W): a 32-channel layer's input and output
    pre-activations (independent: the kernels never ask that z = conv(h)).  prev / cur: their records.
    w[k]: layer k + 1's weights as the model holds them (fp32); wq[k]: rounded to bf16.  dh: the upstream
    gradient of h = relu(BN(z)), as fp32 (``dh32``) and as bf16 (``dh16``) -- the same values on the lattice."""

    def __init__(self, mode: str, U: int, B: int, W: int, seed: int):
        assert mode in ("lattice", "real")
        self.mode, self.U, self.B, self.W, self.seed = mode, U, B, W, seed
        self.N, self.EC, self.HW = U * B, E * CO, H * W
        g = torch.Generator().manual_seed(1000 * seed + 7 * W + 131 * U + B)
        N, EC = self.N, self.EC
        if mode == "lattice":
            ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(D)
            pick = lambda vals, *s: torch.tensor(vals, dtype=D)[torch.randint(0, len(vals), s, generator=g)]
            self.x1 = ri(-3, 3, N, 2 * E, H, W)
            self.z_prev, self.z = ri(-4, 4, N, EC, H, W), ri(-4, 4, N, EC, H, W)
            self.dh32 = ri(-2, 2, N, EC, H, W)
            self.dh16 = self.dh32
            mk = lambda: dict(mean=ri(-1, 1, U, EC), inv=torch.ones(U, EC, dtype=D), a=pick([1., 2., -1., -2.], U, EC),
                              b=ri(-2, 2, U, EC), c1=pick([1., -1.], U, EC), c2=ri(-1, 1, U, EC),
                              c3=pick([0., 1., -1.], U, EC))
            self.prev, self.cur = mk(), mk()
            w32 = lambda: (torch.rand(EC, CO, 3, 3, generator=g) < 1.0 / 6).to(D) * pick([1., -1.], EC, CO, 3, 3)
            self.w = [ri(-2, 2, EC, 2, 3, 3), w32(), w32()]
        else:
            f32 = lambda t: t.to(torch.float32).to(D)
            rn = lambda *s: torch.randn(s, generator=g)
            un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(s, generator=g)
            sg = lambda *s: torch.randint(0, 2, s, generator=g).to(torch.float32) * 2 - 1
            self.x1 = f32(rn(N, 2 * E, H, W))
            self.z_prev, self.z = round_bf16(rn(N, EC, H, W).to(D)), round_bf16(rn(N, EC, H, W).to(D))
            self.dh32 = f32(rn(N, EC, H, W))
            self.dh16 = round_bf16(self.dh32)
            mk = lambda: dict(mean=f32(0.3 * rn(U, EC)), inv=f32(un(0.5, 2.0, U, EC)),
                              a=f32(sg(U, EC) * un(0.5, 1.5, U, EC)), b=f32(un(-0.5, 0.5, U, EC)),
                              c1=f32(sg(U, EC) * un(0.5, 1.5, U, EC)), c2=f32(un(-0.5, 0.5, U, EC)),
                              c3=f32(un(-0.5, 0.5, U, EC)))
            self.prev, self.cur = mk(), mk()
            self.w = [f32(0.4 * rn(EC, 2, 3, 3)), f32(0.1 * rn(EC, CO, 3, 3)), f32(0.1 * rn(EC, CO, 3, 3))]
            # The weight-gradient bound below is a pure summation bound: it takes the kernel's staged h to BE the
            # reference's.  A handful of the 10^5..10^6 values a z + b fall so close to a bf16 rounding boundary
            # that fp32 and float64 evaluation round apart (one such h = 4.5 times a dz of 2.3 is 3.3 times the
            # bound); those z_prev move to the next bf16 value, so every h here has one value in any arithmetic.
            for _ in range(8):
                amb = h_flip_room(self.z_prev, self.prev["a"], self.prev["b"], B) > 0
                if not bool(amb.any()):
                    break
                self.z_prev = torch.where(amb, round_bf16(self.z_prev * (1 + 2.0 ** -7) + 2.0 ** -20), self.z_prev)
            assert not bool((h_flip_room(self.z_prev, self.prev["a"], self.prev["b"], B) > 0).any())
        self.wq = [round_bf16(w) for w in self.w]
        self._fwd, self._bwd = {}, {}

    # ---- forward of layer 1, 2 or 3 (layers 2 / 3 share z_prev and differ in their weights)
    def h_in(self, layer: int) -> torch.Tensor:
        if layer == 1:
            return round_bf16(self.x1)
        return bn_relu(self.z_prev, self.prev["a"], self.prev["b"], self.B)

    def fwd(self, layer: int) -> dict:
        if layer not in self._fwd:
            h, w = self.h_in(layer), self.wq[layer - 1]
            z = conv(h, w)
            zs = round_bf16(z)
            self._fwd[layer] = dict(h=h, z=z, S=conv(h.abs(), w.abs()), s1=group_sums(zs, self.U),
                                    s2=group_sums(zs * zs, self.U))
        return self._fwd[layer]

    def stats_of(self, z_stored: torch.Tensor):
        """(s1, s2, S1, S2) of a stored z (float64): the statistics sums and their absolute-addend sums."""
        z = z_stored.to(D)
        return group_sums(z, self.U), group_sums(z * z, self.U), group_sums(z.abs(), self.U), group_sums(z * z, self.U)

    # ---- backward of layer 1, 2 or 3 for the fp32 or the bf16 copy of dh
    def bwd(self, layer: int, dh_bf16: bool) -> dict:
        key = (layer, bool(dh_bf16))
        if key not in self._bwd:
            dh = self.dh16 if dh_bf16 else self.dh32
            g, xhat, dz = bn_backward(dh, self.z, self.cur, self.B)
            dz = round_bf16(dz)
            h, w = self.h_in(layer), self.wq[layer - 1]
            dx, dw = conv_grads(h, w, dz)
            S_dx, S_dw = conv_grads(h.abs(), w.abs(), dz.abs())
            r1, r2, R1, R2 = bn_partials(g, xhat, self.U)
            self._bwd[key] = dict(g=g, xhat=xhat, dz=dz, h=h, dx=dx, dW=dw, S_dx=S_dx, S_dW=S_dw, red1=r1, red2=r2,
                                  R1=R1, R2=R2)
        return self._bwd[key]

    def prev_partials(self, dx_stored: torch.Tensor):
        """The previous layer's BN backward partials from a stored dx: (sum g', sum g' xhat', and their scales)."""
        p = {k: per_n(self.prev[k], self.B) for k in ("mean", "inv", "a", "b")}
        gate = (p["a"] * self.z_prev + p["b"]) > 0
        dx = dx_stored.to(D)
        g = torch.where(gate, dx, torch.zeros_like(dx))
        f = torch.float32
        xhat = ((self.z_prev.to(f) - p["mean"].to(f)) * p["inv"].to(f)).to(D)
        return bn_partials(g, xhat, self.U)

    # ---- the exactness conditions of the lattice: every intermediate representable in its format
    def check_exact(self, f8: bool = False) -> None:
        assert self.mode == "lattice"
        integer = lambda t: bool(torch.equal(t, t.round()))

        def bf16_ok(name, t):
            assert integer(t) and float(t.abs().max()) <= 256, (name, float(t.abs().max()))

        def sum_ok(name, t):
            assert integer(t) and float(t.abs().max()) < 2 ** 24, (name, float(t.abs().max()))

        for t in (self.x1, self.z_prev, self.z, self.dh32, *self.w):
            assert integer(t) and is_bf16(t)
        for layer in (1, 2, 3):
            f = self.fwd(layer)
            bf16_ok("h", f["h"])
            bf16_ok("z", f["z"])
            # every partial sum of z / z^2, in any order and grouping, is an integer below the sums of |addends|
            sum_ok("sum |z|", group_sums(f["z"].abs(), self.U))
            sum_ok("sum z^2", f["s2"])
            if f8 and layer > 1:
                assert float(f["h"].max()) <= 16 and float(self.w[layer - 1].abs().max()) <= 16
            for dh_bf16 in (False, True):
                b = self.bwd(layer, dh_bf16)
                bf16_ok("dz", b["dz"])
                assert integer(b["xhat"]) and integer(b["g"])
                sum_ok("dW addends", b["S_dW"])
                sum_ok("BN partial addends", b["R1"])
                sum_ok("BN partial addends", b["R2"])
                if layer > 1:
                    bf16_ok("dx", b["dx"])
                    sum_ok("dx addends", b["S_dx"])
                    _, _, P1, P2 = self.prev_partials(b["dx"])
                    sum_ok("previous partial addends", P1)
                    sum_ok("previous partial addends", P2)


@functools.lru_cache(maxsize=None)
def case(mode: str, U: int, B: int, W: int, seed: int = 0) -> Case:
    return Case(mode, U, B, W, seed)


class Impulse(Case):
    """One non-zero pixel at each corner and at one edge midpoint, one non-zero weight per tap: redundant with the
    lattice, but a failure names the tap and the border.  Pixel k (of 5) has the value k + 1 and sits in channels
    0..8 of every expert; tap t is the only non-zero weight of (output channel t, input channel t), so a wrong
    element's channel is the tap and its value the pixel.  Identity records: h = relu(z_prev) = z_prev, dz = dh."""

    PIX = ((0, 0), (0, -1), (-1, 0), (-1, -1), (0, None))   # (row, col); None = the middle column

    def __init__(self, U: int, B: int, W: int):
        Case.__init__(self, "lattice", U, B, W, 99)
        N, EC = self.N, self.EC
        one = torch.ones(U, EC, dtype=D)
        zero = torch.zeros(U, EC, dtype=D)
        # identity records: h = relu(z_prev), dz = dh where z > 0
        self.prev = dict(mean=zero, inv=one, a=one, b=zero, c1=one, c2=zero, c3=zero)
        self.cur = dict(self.prev)
        self.x1, self.z_prev = torch.zeros(N, 2 * E, H, W, dtype=D), torch.zeros(N, EC, H, W, dtype=D)
        self.z = torch.ones(N, EC, H, W, dtype=D)
        self.dh32 = torch.zeros(N, EC, H, W, dtype=D)
        for k, (r, c) in enumerate(self.PIX):
            c = W // 2 if c is None else c
            self.x1[:, :, r, c] = k + 1
            for t in range(9):   # the 5 pixels in channels 0..8 of every expert
                self.z_prev[:, t::CO, r, c] = k + 1
                self.dh32[:, t::CO, r, c] = k + 1
        self.dh16 = self.dh32
        # weight tap t = 3 kh + kw: 1 at (output channel t, input channel t) -- layer 1: input channel t % 2
        self.w = [torch.zeros(EC, 2, 3, 3, dtype=D), torch.zeros(EC, CO, 3, 3, dtype=D), torch.zeros(EC, CO, 3, 3, dtype=D)]
        for t in range(9):
            self.w[0][t::CO, t % 2, t // 3, t % 3] = 1.0
            for k in (1, 2):
                self.w[k][t::CO, t, t // 3, t % 3] = 1.0
        self.wq = [round_bf16(w) for w in self.w]
        self._fwd, self._bwd = {}, {}


@functools.lru_cache(maxsize=None)
def impulse(U: int, B: int, W: int) -> Impulse:
    return Impulse(U, B, W)


# ------------------------------------------------------------------------------------------ BN finalisation
def bn_true_records(z: torch.Tensor, dh: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, U: int, eps: float):
    """Records from TRUE batch statistics, all float64: (mean, inv, a, b) of z per (group, channel) and
    c1 = gamma inv, c2 = c1 mean(g), c3 = c1 mean(g xhat).  z, dh: (N, EC, H, W); gamma, beta: (EC,)."""
    B = z.shape[0] // U
    n = B * z.shape[2] * z.shape[3]
    mean = group_sums(z, U) / n
    var = group_sums(z * z, U) / n - mean * mean
    inv = 1.0 / torch.sqrt(var + eps)
    a = gamma[None, :] * inv
    b = beta[None, :] - mean * a
    rec = dict(mean=mean, inv=inv, a=a, b=b, c1=a.clone(), c2=torch.zeros_like(a), c3=torch.zeros_like(a))
    g, xhat, _ = bn_backward(dh, z, rec, B, D)
    sg, sgx, _, _ = bn_partials(g, xhat, U)
    rec["c2"], rec["c3"] = rec["c1"] * sg / n, rec["c1"] * sgx / n
    return rec, sg, sgx
