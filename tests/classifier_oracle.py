"""Float64 oracle of the scenario classifier kernels (csrc/hip/sc.hip, qsc.hip, qsc_mfma.hip): the operation stage by
stage, the kernels' saved-state encodings, the backward as a linear map of the saved state, lattice and REAL data, the
exactness conditions, the derived per-element bounds, the comparison functions the GPU tests call, and a set of mutants
those comparisons must reject.  Pure torch, any device; a helper module, not a conftest.

The operation, for (H, W) = (16, 8) [pilot 128] and (16, 16) [pilot 256]:

  SC    conv3x3(2 -> 32, no bias) -> ReLU -> pool 2x2 -> conv3x3(32 -> 32, no bias) -> ReLU -> pool
        -> flatten (C, H/4, W/4) -> linear(F -> 3) -> log_softmax, mean NLL, argmax, correct count, dlogit = (softmax - onehot) / B
  QSC   conv3x3(2 -> 16, bias) -> ReLU -> pool -> conv3x3(16 -> 32, bias) -> ReLU -> pool -> flatten
        -> linear(F -> n, bias) -> tanh (angles); head: E Wc^T + bc -> log_softmax, mean NLL, dE, dWc, dbc
  qd_outer_partial   slab[s] = D[chunk s]^T P[chunk s]

ReLU(max(window)) = max(ReLU(window)), so the pooled VALUE is the same whichever comes first; the CHOICE is not: the
QSC kernels pool the ReLU'd values (an all-nonpositive window is a 4-way tie at 0: code 0, torch's max_pool2d index),
sc.hip pools the raw conv outputs (first maximum of the raw values).  ``pool(z, relu_first)`` gives both.  The choice
is the FIRST maximum in scan order TL, TR, BL, BR = 0..3, torch's rule (tests/test_classifier_oracle_cpu.py anchors it
to max_pool2d(return_indices=True)).

Backward conditioned on saved state.  The kernels route gradients through the forward's saved choices and the masks
p1 > 0, p2 > 0; given those the gradient is a linear map, so ``backward`` takes the saved tensors (p1, c1, p2, c2) and
the gradient d3 of the linear layer's pre-activation (dpre = dang (1 - angles^2), or dlogit) and near-ties in the
forward cannot blur the check.

Bounds (all per element, c * S with S the sum of absolute addends of that element, first order in EPS = 2^-24):

  dot     an fp32 sum of K products in ANY order and grouping (VALU chains, v_mfma_f32_* with fp32 operands, wave
          shuffles, per-wave partial rows summed in LDS, slab rows summed afterwards): K - 1 additions and K product
          roundings (none when fused), each at most EPS times a partial sum of magnitude <= S, plus the bias add and
          the final store: (K + 2) EPS S.  K counts the NONZERO addends only (adding an exact zero does not round;
          the routed gradients are three quarters zeros).
  bf16x3  split_bf16 (qsc_mfma.hip): hi = bf16(v), lo = bf16(v - hi).  bf16 keeps 8 significant bits, unit roundoff
          2^-8 (conv_oracle.EPS_BF16): |v - hi| <= 2^-8 |v|, and the residual after lo |r| <= 2^-8 |v - hi| <= 2^-16 |v|.
          The kernels issue ah bh + ah bl + al bh (read at every v_mfma_*_bf16 triple of qsc_mfma.hip); against
          a b = (ah + al + ra) (bh + bl + rb) that drops al bl (<= 2^-16 |a b|), ra b and a rb (<= 2^-16 |a b| each):
          3 * 2^-16 |a b| per product in the worst case, 3 * 2^-16 S per output on top of ``dot`` (the three bf16
          products are exact in the fp32 accumulator).  The kernel header's "relative error ~1e-5" is the typical
          size; 3 * 2^-18, the figure with bf16 taken as a 9-bit format, is exceeded by qd_qsc2_bwd3's dW2 on randn
          data (1.33 of it).  On the lattice ra = rb = 0 needs 16 significant bits per operand, and al bl = 0 needs
          one operand of every product to have 8: ``check_exact`` asks for both (x, the weights and p1 have 8, the
          routed gradients 16).
  carried the error an input of a stage already has, pushed through the stage's absolute linear map (|W| |dx|).
  exp     __expf(x) = v_exp_f32(x * log2(e)): V_EXP_F32 is documented at 1 ULP (AMD Instinct CDNA3/CDNA4 ISA guides,
          VOP1 opcode table), the scaled argument carries the rounding of log2(e) and of the product, 2^-24 |x| each
          in the result: relative 2^-23 (1 + |x|).
  log     __logf(x) = v_log_f32(x) * ln 2: V_LOG_F32 1 ULP (same table), ln 2 and the product one rounding each:
          absolute 2^-22 |ln x|.
  tanh    tanhf is OCML's; OCML is built to the OpenCL full-profile accuracy table (OpenCL C specification, "Relative
          error as ULPs": tanh <= 5 ulp): 5 * 2^-23 |tanh z| plus the carried error of z (|tanh'| <= 1).
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from conv_oracle import D, EPS_F32, is_f32, worst_ratio  # noqa: F401

EPS = EPS_F32
X3 = 3 * 2.0 ** -16          # the bf16x3 term per product (see the module docstring)
TANH_ULPS = 5
GEOS = {128: (16, 8), 256: (16, 16)}
ALIGN = 16                   # FlatParamSpace's alignment of every tensor, in floats
I64 = torch.int64

SC = NS(name="sc", c1=32, c2=32, bias=False, relu_first=False)
QSC = NS(name="qsc", c1=16, c2=32, bias=True, relu_first=True)


def feat(H: int, W: int) -> int:
    return 32 * (H // 4) * (W // 4)


# ------------------------------------------------------------------------------------------ stages (float64)
def conv(x, w, b=None, dt=D):
    return F.conv2d(x.to(dt), w.to(dt), None if b is None else b.to(dt), padding=1)


def conv_S(x, w, b=None):
    """Sum of absolute addends of every conv output, and the count of nonzero ones."""
    S = F.conv2d(x.to(D).abs(), w.to(D).abs(), None if b is None else b.to(D).abs(), padding=1)
    K = F.conv2d((x != 0).to(D), (w != 0).to(D), padding=1)
    return S, K


def windows(z):
    """(B, C, H, W) -> (B, C, H/2, W/2, 4): each 2x2 window in scan order TL, TR, BL, BR."""
    return torch.stack((z[..., 0::2, 0::2], z[..., 0::2, 1::2], z[..., 1::2, 0::2], z[..., 1::2, 1::2]), dim=-1)


def first_max(w, last: bool = False):
    """Index of the first (``last``: last -- a mutant) maximum along the last dimension."""
    m = w.amax(-1, keepdim=True)
    k = torch.arange(w.shape[-1], device=w.device)
    if last:
        return torch.where(w == m, k, -1).amax(-1)
    return torch.where(w == m, k, w.shape[-1]).amin(-1)


def pool(z, relu_first: bool, last: bool = False):
    """ReLU + 2x2 max pool of the pre-activations z: (pooled value, choice code 0..3)."""
    w = windows(z)
    code = first_max(torch.relu(w) if relu_first else w, last)
    return torch.relu(w.amax(-1)), code


def unpool(g, code):
    """Routes g (B, C, h, w) to position ``code`` of every 2x2 window: (B, C, 2h, 2w), zeros elsewhere."""
    B, C, h, w = g.shape
    out = torch.zeros(B, C, 2 * h, 2 * w, dtype=g.dtype, device=g.device)
    for k in range(4):
        out[..., k >> 1::2, k & 1::2] = torch.where(code == k, g, torch.zeros_like(g))
    return out


def linear(p, w, b=None, dt=D):
    """p (B, F), w (n, F): (z, S, K)."""
    z = p.to(dt) @ w.to(dt).T
    p, w = p.to(D), w.to(D)
    S = p.abs() @ w.abs().T
    K = (p != 0).to(D) @ (w != 0).to(D).T
    if b is not None:
        z, S = z + b.to(dt), S + b.to(D).abs()
    return z, S, K


def dot_bound(K, S, x3: bool = False, carried=0.0, depth=None):
    """``dot`` of the module docstring.  depth: the longest chain of additions any addend of the kernel's sum passes
    through, where the kernel that is read fixes it (a per-lane chain, then a shuffle tree): no addend is rounded
    more often than that, so min(K, depth) takes K's place."""
    if depth is not None:
        K = torch.clamp(K, max=depth) if torch.is_tensor(K) else min(K, depth)
    return (K + 2) * EPS * S + (X3 * S if x3 else 0.0) + carried


def linear_depth(kernel: str, F_: int) -> int:
    """The linear layer's summation depth, read off the three forward kernels:
    qsc2 (qsc_mfma.hip qsc2_fwd_kernel): 4 lanes per output, F/4 fused multiply-adds each, 2 shuffle adds, the bias;
    qsc  (qsc.hip sample_forward): F/256 per thread, wave_sum's 6 levels, the 4 waves' partials and the bias (4 adds);
    sc   (sc.hip sc_fwd_kernel): F/256 per thread, wave_sum's 6 levels, 4 waves (4 adds from 0), the bias."""
    return {"qsc2": F_ // 4 + 3, "qsc": F_ // 256 + 10, "sc": F_ // 256 + 11}[kernel]


def tanh_bound(z, ez):
    return TANH_ULPS * 2.0 ** -23 * torch.tanh(z).abs() + ez


def exp_rel(x):
    return 2.0 ** -23 * (1 + x.abs())


def softmax_head(logits, el, labels=None, inv_b=None):
    """log_softmax and what follows, in float64, with the bounds of an fp32 evaluation through __expf / __logf whose
    logits are within ``el`` of these: NS(logp, b_logp, pred, [nll, b_nll, dlogit, b_dlogit])."""
    l = logits.to(D)
    m = l.amax(1, keepdim=True)
    a = l - m
    se = a.exp().sum(1, keepdim=True)
    lse = m + se.log()
    logp = l - lse
    C = l.shape[1]
    dl = el.amax(1, keepdim=True) if torch.is_tensor(el) else el
    rel_se = (exp_rel(a) + EPS * a.abs()).amax(1, keepdim=True) + (C - 1) * EPS
    b_logp = 2 * dl + rel_se + 2.0 ** -22 * se.log().abs() + EPS * (lse.abs() + logp.abs()) + 0 * logp
    out = NS(logits=l, el=el, logp=logp, b_logp=b_logp, pred=l.argmax(1))
    if labels is not None:
        y = labels.to(l.device).to(I64)
        oh = F.one_hot(y, C).to(D)
        p = logp.exp()
        out.nll = -(logp * oh).sum(1)
        out.b_nll = (b_logp * oh).sum(1)
        out.dlogit = (p - oh) * inv_b
        out.b_dlogit = (p * (exp_rel(logp) + b_logp) + 3 * EPS * (p - oh).abs()) * inv_b
    return out


def argmax_ok(pred, ref: NS):
    """A kernel argmax that differs from float64's is accepted only where the two logits lie within their bounds."""
    pred = pred.to(ref.logits.device).to(I64)
    lk = ref.logits.gather(1, pred[:, None])[:, 0]
    lo = ref.logits.amax(1)
    el = ref.el if torch.is_tensor(ref.el) else torch.full_like(ref.logits, ref.el)
    room = el.gather(1, pred[:, None])[:, 0] + el.gather(1, ref.pred[:, None])[:, 0]
    return (pred == ref.pred) | (lo - lk <= room)


# ------------------------------------------------------------------------------------------ forward
def forward(net, x, P, p1=None, p2=None, x3: bool = False, dt=D, depth3=None):
    """Every stage in float64.  p1 / p2 (optional, (B, C, h, w)): the values the later stages read instead of this
    oracle's own -- a kernel's saved maps, so that each stage is checked on the inputs the kernel really had.
    dt = float32: the values (not S, K and the bounds) in eager fp32, for the CPU tests of the bounds."""
    r = NS()
    r.z1 = conv(x, P["w1"], P.get("b1"), dt)
    r.S1, r.K1 = conv_S(x, P["w1"], P.get("b1"))
    r.p1, r.c1 = pool(r.z1, net.relu_first)
    q1 = r.p1 if p1 is None else p1
    r.z2 = conv(q1, P["w2"], P.get("b2"), dt)
    r.S2, r.K2 = conv_S(q1, P["w2"], P.get("b2"))
    r.p2, r.c2 = pool(r.z2, net.relu_first)
    q2 = r.p2 if p2 is None else p2
    r.z3, r.S3, r.K3 = linear(q2.flatten(1), P["wl"], P.get("bl"), dt)
    r.b1 = dot_bound(r.K1, r.S1)
    r.b2 = dot_bound(r.K2, r.S2, x3)
    r.b3 = dot_bound(r.K3, r.S3, depth=depth3)
    return r


# ------------------------------------------------------------------------------------------ backward
_DT = [D]


class _dtype:
    """Evaluate ``backward`` in another dtype (its bounds are then meaningless: only .g is kept)."""

    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        _DT[0] = self.dt

    def __exit__(self, *a):
        _DT[0] = D


def _wgrad(xin, dz, e_dz=None, pad_mode: str = "constant", e_x=None):
    """dW (Co, Cin * 9) = sum over samples and positions of dz (x) im2col(xin), with S, the nonzero-addend count K
    and the carried error of dz."""
    U = F.unfold(F.pad(xin, (1, 1, 1, 1), mode=pad_mode), 3)
    f = dz.flatten(2)
    e = lambda a, b: torch.einsum("bop,bkp->ok", a, b)
    car = e(e_dz.flatten(2), U.abs()) if e_dz is not None else 0.0
    if e_x is not None:
        car = car + e(f.abs(), F.unfold(F.pad(e_x, (1, 1, 1, 1)), 3))
    return e(f, U), e(f.abs(), U.abs()), e((f != 0).to(_DT[0]), (U != 0).to(_DT[0])), car


def backward(net, x, P, p1, c1, p2, c2, d3, e3=None, x3: bool = False, mutant: str = "", dt=D, e_p1=None, e_p2=None):
    """Gradients of every parameter given the saved state (p1, c1 (B, C1, H/2, W/2); p2, c2 (B, C2, H/4, W/4)) and
    d3 (B, n) = dL / d(linear pre-activation).  e3: the error d3 already carries; e_p1 / e_p2: the error of the maps a
    kernel that recomputes its forward (qsc.hip) has in place of p1 / p2 (their masks and choices taken as equal:
    ``near_ties`` must be 0 for such data).  Returns NS(g, S, bound): dicts over
    w1, b1, w2, b2, wl, bl (no b1 / b2 for a net without conv biases).  ``mutant``: a wrong backward, for the tests
    of the comparison functions."""
    if dt != D:      # the values in eager fp32 (the CPU tests of the bounds); S, K and the bounds come from float64
        v = backward(net, x, P, p1, c1, p2, c2, d3, mutant=mutant)
        with _dtype(dt):
            v.g = backward(net, x, P, p1, c1, p2, c2, d3, mutant=mutant).g
        return v
    dt = _DT[0]
    x, p1, p2, d3 = x.to(dt), p1.to(dt), p2.to(dt), d3.to(dt)
    w2, wl = P["w2"].to(dt), P["wl"].to(dt)
    if mutant == "drop_last_sample":
        d3 = d3.clone()
        d3[-1] = 0
    e3 = torch.zeros_like(d3) if e3 is None else e3.to(_DT[0])
    g, S, bd = {}, {}, {}
    pf = p2.flatten(1)
    g["wl"], S["wl"] = d3.T @ pf, d3.abs().T @ pf.abs()
    Kwl = (d3 != 0).to(_DT[0]).T @ (pf != 0).to(_DT[0])
    car = e3.T @ pf.abs() + (d3.abs().T @ e_p2.flatten(1) if e_p2 is not None else 0.0)
    bd["wl"] = dot_bound(Kwl, S["wl"], carried=car)
    g["bl"], S["bl"] = d3.sum(0), d3.abs().sum(0)
    bd["bl"] = dot_bound((d3 != 0).to(_DT[0]).sum(0), S["bl"], carried=e3.sum(0))
    # pool-2 / ReLU backward
    m2 = (pf >= 0) if mutant == "grad_at_zero" else (pf > 0)
    dp2 = torch.where(m2, d3 @ wl, torch.zeros_like(pf))
    b_dp2 = dot_bound((d3 != 0).to(_DT[0]) @ (wl != 0).to(_DT[0]), d3.abs() @ wl.abs(), carried=e3 @ wl.abs())
    e_dp2 = torch.where(m2, b_dp2, torch.zeros_like(pf))
    dz2, e_dz2 = unpool(dp2.view_as(p2), c2), unpool(e_dp2.view_as(p2), c2)
    g["w2"], S["w2"], K, car = _wgrad(p1, dz2, e_dz2, "replicate" if mutant == "pad_ring" else "constant", e_p1)
    bd["w2"] = dot_bound(K, S["w2"], x3, car)
    if net.bias:
        g["b2"], S["b2"] = dz2.sum((0, 2, 3)), dz2.abs().sum((0, 2, 3))
        bd["b2"] = dot_bound((dz2 != 0).to(_DT[0]).sum((0, 2, 3)), S["b2"], carried=e_dz2.sum((0, 2, 3)))
        if mutant == "no_b2":
            g["b2"] = torch.zeros_like(g["b2"])
    # conv2 data gradient, pool-1 / ReLU backward
    if mutant == "unflipped":
        dp1 = F.conv2d(dz2, w2.transpose(0, 1), padding=1)
    else:
        dp1 = F.conv_transpose2d(dz2, w2, padding=1)
    S_dp1 = F.conv_transpose2d(dz2.abs(), w2.abs(), padding=1)
    K_dp1 = F.conv_transpose2d((dz2 != 0).to(_DT[0]), (w2 != 0).to(_DT[0]), padding=1)
    m1 = p1 > 0
    zero = torch.zeros_like(dp1)
    e_dp1 = torch.where(m1, dot_bound(K_dp1, S_dp1, x3, F.conv_transpose2d(e_dz2, w2.abs(), padding=1)), zero)
    dp1 = torch.where(m1, dp1, zero)
    dz1, e_dz1 = unpool(dp1, c1), unpool(e_dp1, c1)
    g["w1"], S["w1"], K, car = _wgrad(x, dz1, e_dz1)
    bd["w1"] = dot_bound(K, S["w1"], x3, car)
    if net.bias:
        g["b1"], S["b1"] = dz1.sum((0, 2, 3)), dz1.abs().sum((0, 2, 3))
        bd["b1"] = dot_bound((dz1 != 0).to(_DT[0]).sum((0, 2, 3)), S["b1"], carried=e_dz1.sum((0, 2, 3)))
    return NS(g=g, S=S, bound=bd, dz2=dz2, dz1=dz1, dp2=dp2)


def dpre(angles, dang, mutant: str = ""):
    """dL/d(pre-tanh) = dang (1 - angles^2) and its fp32 bound: a^2 (or the fused 1 - a^2), the subtraction and the
    product, three roundings of values <= |dang|."""
    a, d = angles.to(D), dang.to(D)
    v = d * ((1 - a) if mutant == "one_minus_a" else (1 - a * a))
    return v, 3 * EPS * d.abs() * (1 + a * a)


# ------------------------------------------------------------------------------------------ heads, outer product
def head(E, wc, bc, labels, Bdiv=None, depth=None):
    """QSC head: NS of softmax_head's fields plus loss, dE, dWc, dbc and their bounds."""
    E, wc = E.to(D), wc.to(D)
    B = E.shape[0]
    lg, S, K = linear(E, wc, bc)
    r = softmax_head(lg, dot_bound(K, S), labels, 1.0 / (Bdiv or B))
    if labels is not None:
        gl, eg = r.dlogit, r.b_dlogit
        r.loss = r.nll.sum() / B
        r.b_loss = (r.b_nll.sum() + (min(B, depth or B) + 2) * EPS * r.nll.abs().sum()) / B
        r.dE = gl @ wc
        r.b_dE = dot_bound(wc.shape[0], gl.abs() @ wc.abs(), carried=eg @ wc.abs())
        r.dWc = gl.T @ E
        r.b_dWc = dot_bound(B, gl.abs().T @ E.abs(), carried=eg.T @ E.abs(), depth=depth)
        r.dbc = gl.sum(0)
        r.b_dbc = dot_bound(B, gl.abs().sum(0), carried=eg.sum(0), depth=depth)
    return r


def outer_partial(Dm, Pm, bs: int):
    """slab (S, n, F) = per-chunk D^T P, its sums of absolute addends and bounds."""
    Dm, Pm = Dm.to(D), Pm.to(D)
    g, bd = [], []
    for b0 in range(0, Dm.shape[0], bs):
        d, p = Dm[b0:b0 + bs], Pm[b0:b0 + bs]
        g.append(d.T @ p)
        bd.append(dot_bound((d != 0).to(D).T @ (p != 0).to(D), d.abs().T @ p.abs()))
    return torch.stack(g), torch.stack(bd)


# ------------------------------------------------------------------------------------------ codecs
def enc_p1s(p1):
    """(B, 16, h, w) -> the MFMA path's channel-last (B, h * w, 16)."""
    return p1.permute(0, 2, 3, 1).reshape(p1.shape[0], -1, p1.shape[1]).contiguous()


def dec_p1s(p1s, h: int, w: int):
    B = p1s.shape[0]
    return p1s.reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


def enc_c1(code):
    """(B, 16, h, w) codes -> (B, h * w) int32 words (the kernel's uint32), 2 bits per channel: bits 2c, 2c + 1."""
    B, C = code.shape[:2]
    sh = (2 * torch.arange(C, device=code.device)).view(1, C, 1)
    v = (code.reshape(B, C, -1).to(I64) << sh).sum(1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def dec_c1(c1, h: int, w: int, C: int = 16):
    v = c1.to(I64) & 0xFFFFFFFF
    sh = (2 * torch.arange(C, device=c1.device)).view(1, C, 1)
    return ((v.unsqueeze(1) >> sh) & 3).reshape(c1.shape[0], C, h, w)


def enc_u8(code):
    """(B, C, h, w) codes -> (B, C * h * w) uint8 (sc.hip's c1s / c2s, the MFMA path's c2)."""
    return code.reshape(code.shape[0], -1).to(torch.uint8)


def dec_u8(c, C: int, h: int, w: int):
    return c.to(I64).reshape(c.shape[0], C, h, w)


# ------------------------------------------------------------------------------------------ flat layouts
def _up(v: int, a: int = ALIGN) -> int:
    return -(-v // a) * a


def qsc_layout(n: int, F_: int, qwidth: int = 0, q_first: bool = True, lead: int = 0):
    """A flat buffer as FlatParamSpace lays one out (every tensor on a 16-float boundary): the preprocess parameters
    w1 b1 w2 b2 wl bl and ``qwidth`` quantum weights before or after them, ``lead`` unused floats in front.  Returns
    NS(off: dict, numel, base, row, offs: the kernels' 9-int array as a list, ranges: name -> (start, length))."""
    sizes = [("w1", 288), ("b1", 16), ("w2", 4608), ("b2", 32), ("wl", n * F_), ("bl", n)]
    q = [("qw", qwidth)] if qwidth else []
    order = (q + sizes) if q_first else (sizes + q)
    off, pos = {}, _up(lead)
    for k, s in order:
        off[k] = pos
        pos = _up(pos + s)
    if "qw" not in off:
        off["qw"] = off["w1"]      # (never read: the kernels look at it only with a quantum slab)
    base = min(off["w1"], off["qw"]) if qwidth else off["w1"]
    end = max(off["bl"] + n, off["qw"] + qwidth)
    row = _up(end - base, 4)
    numel = _up(base + row)
    offs = [off[k] for k, _ in sizes] + [row, base, off["qw"]]
    ranges = {k: (off[k], s) for k, s in sizes}
    if qwidth:
        ranges["qw"] = (off["qw"], qwidth)
    return NS(off=off, numel=numel, base=base, row=row, offs=offs, ranges=ranges)


def sc_layout(F_: int):
    off = {"w1": 0, "w2": 576, "wl": 576 + 9216, "bl": 576 + 9216 + 3 * F_}
    row = off["bl"] + 16
    return NS(off=off, numel=row, base=0, row=row, offs=[off["w1"], off["w2"], off["wl"], off["bl"], row],
              ranges={"w1": (0, 576), "w2": (576, 9216), "wl": (off["wl"], 3 * F_), "bl": (off["bl"], 3)})


def pack(lay, P, fill: float = 0.0):
    """The fp32 flat buffer holding the parameters P at the layout's offsets (``fill`` in the gaps)."""
    flat = torch.full((lay.numel,), fill, dtype=torch.float32)
    for k, (o, s) in lay.ranges.items():
        if k in P:
            flat[o:o + s] = P[k].reshape(-1).to(torch.float32)
    return flat


def row_of(lay, vals: dict, dtype=D):
    """A slab row (columns [base, base + row)) with ``vals`` at their ranges and zeros elsewhere."""
    r = torch.zeros(lay.row, dtype=dtype)
    for k, v in vals.items():
        o, s = lay.ranges[k]
        r[o - lay.base:o - lay.base + s] = v.reshape(-1).to(dtype).cpu()
    return r


def gap_columns(lay, absent=()):
    """Boolean (row,): the columns of a slab row that belong to no parameter (alignment gaps and the tail) or to a
    parameter in ``absent`` (wl when the kernel leaves it to the GEMM, qw without a quantum slab): exactly +0."""
    m = torch.ones(lay.row, dtype=torch.bool)
    for k, (o, s) in lay.ranges.items():
        if k not in absent:
            m[max(o - lay.base, 0):max(o - lay.base + s, 0)] = False
    return m


# ------------------------------------------------------------------------------------------ data
def _gen(*key) -> torch.Generator:
    s = 12345
    for d in key:
        s = (s * 1000003 + (d if isinstance(d, int) else sum(map(ord, str(d))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(g, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(D)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v


MASTER_B = 16   # samples of a lattice master set; a case of B samples takes the first B


@functools.lru_cache(maxsize=None)
def _convs(netname: str, pilot: int, mode: str, seed: int):
    """x (MASTER_B, 2, H, W) and the conv parameters of one (net, geometry, mode): shared by every B and n."""
    net = SC if netname == "sc" else QSC
    H, W = GEOS[pilot]
    g = _gen(netname, pilot, mode, seed)
    P = {}
    if mode == "lattice":
        x = _ints(g, (MASTER_B, 2, H, W), -2, 2)
        flatw = torch.rand((MASTER_B, H // 2, W // 2), generator=g) < 0.15      # channel 1: some constant windows
        lvl = _ints(g, (MASTER_B, H // 2, W // 2), -2, 2)
        x[:, 1] = torch.where(flatw.repeat_interleave(2, 1).repeat_interleave(2, 2),
                              lvl.repeat_interleave(2, 1).repeat_interleave(2, 2), x[:, 1])
        P["w1"] = _ints(g, (net.c1, 2, 3, 3), -2, 2, 0.3)
        P["w2"] = _ints(g, (net.c2, net.c1, 3, 3), -1, 1, 0.08)
        for co in range(8):       # the copy channels: centre tap +-1 on one input channel
            neg = co in (4, 6, 7) if not net.bias else co in (6, 7)
            P["w1"][co] = 0
            P["w1"][co, co % 2, 1, 1] = -1 if neg else 1
            P["w2"][co] = 0
            P["w2"][co, co, 1, 1] = -1 if neg else 1
        if net.bias:
            P["b1"] = _ints(g, (net.c1,), -2, 2)
            P["b2"] = _ints(g, (net.c2,), -2, 2)
            P["b1"][:8] = torch.tensor([0, 0, -1, 1, -4, 0, 0, 2.0], dtype=D)
            P["b2"][:8] = torch.tensor([0, -1, 0, -2, -300, 0, 0, 2.0], dtype=D)
    else:
        x = torch.randn((MASTER_B, 2, H, W), generator=g)
        u = lambda shape, fan: (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan)
        k = 3.0 if netname == "sc" else 1.0
        P["w1"] = u((net.c1, 2, 3, 3), 18) * k
        P["w2"] = u((net.c2, net.c1, 3, 3), 9 * net.c1) * k
        if net.bias:
            P["b1"], P["b2"] = u((net.c1,), 18), u((net.c2,), 9 * net.c1)
    return x.to(torch.float32).to(D), {k_: v.to(torch.float32).to(D) for k_, v in P.items()}


@functools.lru_cache(maxsize=None)
def case(netname: str, pilot: int, B: int, n: int, mode: str, seed: int = 0):
    """Inputs x (B, 2, H, W), parameters P and labels of one data set, float64 values that fp32 holds exactly.

    LATTICE: integers.  x in -2..2 (channel 1 with some constant 2x2 windows: the 4-way ties of pool 1); conv
    weights sparse small integers; the first eight output channels of both
    convs copy one input channel (centre tap +-1, integer bias): their windows repeat the few levels of their input,
    which gives the ties, zeros and all-negative windows random data never has (``window_cases`` counts them on the
    master set of MASTER_B samples; a case of B samples is its first B, so every case is a part of a set that has
    them all and the largest cases hold nearly all).  The linear layer: sparse {-1, 0, 1} 2^-6 (2^-5 for SC), so that
    F = 256 / 512 addends stay small and tanh / softmax unsaturated.  The backward lattice (QSC): angles in
    {0, +-1/2}, integer dang; (SC): dlogit in multiples of 2^-4.
    REAL: randn inputs, default-init-style weights (uniform +-1/sqrt(fan_in); SC x3 for live ReLUs)."""
    assert B <= MASTER_B
    net = SC if netname == "sc" else QSC
    H, W = GEOS[pilot]
    F_ = feat(H, W)
    xm, Pc = _convs(netname, pilot, mode, seed)
    g = _gen(netname, pilot, B, n, mode, seed)
    P = dict(Pc)
    if mode == "lattice":
        ul = 2.0 ** (-5 if netname == "sc" else -6)
        P["wl"] = _ints(g, (n, F_), -1, 1, 0.1) * ul
        P["bl"] = _ints(g, (n,), -8, 8) * ul
    else:
        k = 3.0 if netname == "sc" else 1.0
        u = lambda shape, fan: ((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan) * k).to(torch.float32).to(D)
        P["wl"], P["bl"] = u((n, F_), F_), u((n,), F_)
    labels = torch.randint(0, 3, (B,), generator=g)
    c = NS(net=net, pilot=pilot, H=H, W=W, F=F_, B=B, n=n, mode=mode, x=xm[:B].clone(), P=P, labels=labels, seed=seed)
    if mode == "lattice":
        c.angles = _ints(g, (B, n), -1, 1) * 0.5
        c.dang = _ints(g, (B, n), -2, 2)
        c.dlogit = _ints(g, (B, n), -4, 4) * 2.0 ** -4
    else:
        c.angles = torch.tanh(torch.randn((B, n), generator=g)).to(torch.float32).to(D)
        c.dang = torch.randn((B, n), generator=g).to(torch.float32).to(D)
        c.dlogit = (torch.randn((B, n), generator=g) / B).to(torch.float32).to(D)
    return c


def master(c):
    """The MASTER_B-sample set a lattice case is the head of (same parameters)."""
    return case(c.net.name, c.pilot, MASTER_B, c.n, c.mode, c.seed)


# ------------------------------------------------------------------------------------------ exactness, case counts
def has_bits(x, nbits: int) -> bool:
    """Every value has at most ``nbits`` significant bits (is its own bf16 hi for 8, its hi + lo for 16)."""
    b = x.to(D).contiguous().view(I64)
    return bool(((b & ((1 << (53 - nbits)) - 1)) == 0).all())


def on_lattice(x, unit: float) -> bool:
    q = x.to(D) / unit
    return bool((q == q.round()).all())


def check_exact(c, x3: bool = True):
    """The lattice conditions of data set c, from the oracle's own S: every sum of absolute addends stays below 2^24
    units of the lattice spacing of its stage (then every partial sum any kernel variant forms is an integer multiple
    of the unit below 2^24 units: exact in fp32), and for the bf16x3 variants every product has one operand of 8
    significant bits and one of 16 (see the module docstring).  Returns the forward and backward oracle results."""
    net, P = c.net, c.P
    ul = 2.0 ** (-5 if net.name == "sc" else -6)
    r = forward(net, c.x, P)
    for nm, S, unit in (("conv1", r.S1, 1.0), ("conv2", r.S2, 1.0), ("linear", r.S3, ul)):
        assert float(S.max()) / unit < 2 ** 24, (nm, float(S.max()))
    assert on_lattice(c.x, 1) and on_lattice(P["w1"], 1) and on_lattice(P["w2"], 1) and on_lattice(P["wl"], ul)
    if net.name == "sc":
        d3, ud = c.dlogit, 2.0 ** -4
    else:
        d3, _ = dpre(c.angles, c.dang)
        ud = 0.25
        assert bool(((c.angles * 2).abs() <= 1).all()) and on_lattice(c.angles, 0.5) and on_lattice(c.dang, 1)
    assert on_lattice(d3, ud)
    bk = backward(net, c.x, P, r.p1, r.c1, r.p2, r.c2, d3)
    ug = ud * ul                                  # the spacing of dp2 and of everything routed from it
    for k, S in bk.S.items():
        unit = ud if k in ("wl", "bl") else ug
        assert on_lattice(bk.g[k], unit), k
        assert float(S.max()) / unit < 2 ** 24, (k, float(S.max()) / unit)
    if x3:
        for nm, v in (("x", c.x), ("w1", P["w1"]), ("w2", P["w2"]), ("p1", r.p1)):
            assert has_bits(v, 8), nm
        for nm, v in (("dz2", bk.dz2), ("dz1", bk.dz1)):
            assert has_bits(v, 16), nm
    return r, bk


def window_cases(z, relu_first: bool) -> dict:
    """Counts, over the 2x2 windows of the pre-activations z, of the cases a lattice must contain."""
    w = windows(z)
    m = w.amax(-1, keepdim=True)
    ties = (w == m).sum(-1)
    pos = m[..., 0] > 0
    code = first_max(torch.relu(w) if relu_first else w)
    out = {f"tie{k}_at_positive_max": int(((ties == k) & pos).sum()) for k in (2, 3, 4)}
    out["max_exactly_zero"] = int((m[..., 0] == 0).sum())
    out["all_negative"] = int((m[..., 0] < 0).sum())
    for k in range(4):
        out[f"unique_max_at_{k}"] = int(((ties == 1) & pos & (code == k)).sum())
    return out


def check_cases(c, minimum: int = 32):
    """A lattice data set cannot be vacuous: at least ``minimum`` windows of every case in each pool."""
    m = master(c)
    r = forward(m.net, m.x, m.P)
    for nm, z in (("pool1", r.z1), ("pool2", r.z2)):
        for k, v in window_cases(z, m.net.relu_first).items():
            assert v >= minimum, (m.net.name, m.pilot, nm, k, v)


def near_ties(z, bz, relu_first: bool):
    """How many windows of z have a runner-up (or, for the ReLU mask, a zero) within the sum of the two candidates'
    bounds of the maximum: where an fp32 forward may legitimately choose differently."""
    w, b = windows(z), windows(bz)
    m, k = w.max(-1, keepdim=True)
    bm = b.gather(-1, k)
    close = (m - w <= b + bm)
    close.scatter_(-1, k, False)
    # (with the ReLU first a dead window's choice is 0 whatever its values)
    live = (m > -bm)[..., 0] if relu_first else torch.ones_like(m[..., 0], dtype=torch.bool)
    return int((close.any(-1) & live).sum()) + int((m.abs() <= bm).sum())


# ------------------------------------------------------------------------------------------ comparisons
class Check:
    """Collects the comparisons of one test: failures as messages, the achieved max |err| / bound per quantity."""

    def __init__(self, case_name: str = ""):
        self.case, self.fails, self.ratios, self.n = case_name, [], {}, 0

    def equal(self, what, got, ref, bits: bool = False):
        """Exact equality of the values (NaN never equal); ``bits``: of the fp32 bit patterns too (signed zeros)."""
        self.n += 1
        got, ref = got.detach().cpu(), ref.detach().cpu()
        if got.shape != ref.shape:
            self.fails.append(f"{what} {self.case}: shape {tuple(got.shape)} vs {tuple(ref.shape)}")
            return
        if bits:
            bad = got.to(torch.float32).view(torch.int32) != ref.to(torch.float32).view(torch.int32)
        else:
            bad = ~(got.to(D) == ref.to(D)) if got.is_floating_point() else got.to(I64) != ref.to(I64)
        if bool(bad.any()):
            i = bad.flatten().nonzero()[0, 0].item()
            self.fails.append(f"{what} {self.case}: {int(bad.sum())} of {bad.numel()} differ, first at flat index {i}: "
                              f"got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r}")

    def within(self, what, got, ref, bound):
        """Per element |got - ref| <= bound; records the worst ratio."""
        self.n += 1
        got, ref, bound = got.detach().cpu().to(D), ref.detach().cpu().to(D), bound.detach().cpu().to(D)
        if got.shape != ref.shape:
            self.fails.append(f"{what} {self.case}: shape {tuple(got.shape)} vs {tuple(ref.shape)}")
            return
        bound = bound.expand_as(ref)
        r = worst_ratio((got - ref).abs(), bound)
        self.ratios[what] = max(self.ratios.get(what, 0.0), r) if r == r else r
        print(f"ERRBOUND {what} {self.case} {r:.4f}")
        if not r <= 1.0:
            q = ((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).flatten()
            i = int(q.argmax())
            self.fails.append(f"{what} {self.case}: max err / bound = {r} at flat index {i}: got {float(got.flatten()[i])}"
                              f" ref {float(ref.flatten()[i])} bound {float(bound.flatten()[i])}")

    def choices(self, what, code, z, bz, relu_first: bool):
        """A kernel's window choices against the float64 pre-activations z (bounds bz): a choice that differs from
        the oracle's passes only if the float64 value at the kernel's position is within the sum of the two
        candidates' bounds of the float64 maximum.  No mismatch fraction."""
        self.n += 1
        w, b = windows(z), windows(bz)
        if relu_first:
            w = torch.relu(w)
        ref = first_max(w)
        code = code.to(w.device).to(I64)
        if bool(((code < 0) | (code > 3)).any()):
            self.fails.append(f"{what} {self.case}: a code outside 0..3")
            return
        vk, bk = w.gather(-1, code[..., None])[..., 0], b.gather(-1, code[..., None])[..., 0]
        vo, bo = w.gather(-1, ref[..., None])[..., 0], b.gather(-1, ref[..., None])[..., 0]
        bad = (code != ref) & ~(vo - vk <= bk + bo)
        differ = int((code != ref).sum())
        print(f"CHOICES {what} {self.case} differ {differ} of {code.numel()} rejected {int(bad.sum())}")
        if bool(bad.any()):
            i = bad.flatten().nonzero()[0, 0].item()
            self.fails.append(f"{what} {self.case}: {int(bad.sum())} choices differ beyond a near-tie, first at window "
                              f"{i}: kernel {int(code.flatten()[i])} oracle {int(ref.flatten()[i])}")

    def true(self, cond, msg):
        self.n += 1
        if not cond:
            self.fails.append(f"{msg} {self.case}")

    def done(self):
        assert self.n > 0
        assert not self.fails, "\n".join(self.fails[:20])


def check_forward_state(chk: Check, net, lattice: bool, r, p1, c1, p2, c2, tag: str = ""):
    """A kernel's saved maps and choices (decoded to (B, C, h, w)) against the forward oracle r, which must have been
    evaluated on the kernel's own p1 / p2 for REAL data (``forward(..., p1=, p2=)``)."""
    if lattice:
        chk.equal(tag + "p1", p1, r.p1)
        chk.equal(tag + "c1", c1, r.c1)
        chk.equal(tag + "p2", p2, r.p2)
        chk.equal(tag + "c2", c2, r.c2)
    else:
        chk.within(tag + "p1", p1, r.p1, windows(r.b1).amax(-1))
        chk.choices(tag + "c1", c1, r.z1, r.b1, net.relu_first)
        chk.within(tag + "p2", p2, r.p2, windows(r.b2).amax(-1))
        chk.choices(tag + "c2", c2, r.z2, r.b2, net.relu_first)


def check_backward(chk: Check, lay, lattice: bool, bk, slab, absent=(), dpre_got=None, dpre_ref=None, tag: str = "",
                   extra: dict = None):
    """A backward kernel's slab (rows, row) against the backward oracle bk.  The rows are summed in float64 (exact on
    the lattice, and adding no error of its own elsewhere).  Every column is covered: the parameters' per element
    (equal on the lattice, within bound otherwise), every other column exactly +0 in every row, no NaN left.
    ``extra``: name -> exact float64 column sums of further ranges (the quantum-slab fold)."""
    slab = slab.detach().cpu()
    chk.true(not bool(torch.isnan(slab).any()), tag + "slab: elements left unwritten (NaN)")
    tot = slab.to(D).sum(0)
    for k, (o, s) in lay.ranges.items():
        if k in absent or (k == "qw" and not extra):
            continue
        got = tot[o - lay.base:o - lay.base + s]
        if extra and k in extra:
            chk.equal(tag + "d" + k, got, extra[k].reshape(-1))
            continue
        ref = bk.g[k].reshape(-1)
        if lattice:
            chk.equal(tag + "d" + k, got, ref)
        else:
            chk.within(tag + "d" + k, got, ref, bk.bound[k].reshape(-1))
    gaps = gap_columns(lay, tuple(absent) + (() if extra else ("qw",)))
    if bool(gaps.any()):
        z = slab[:, gaps]
        chk.equal(tag + "gap columns", z, torch.zeros_like(z), bits=True)
    if dpre_got is not None:
        if lattice:
            chk.equal(tag + "dpre", dpre_got, dpre_ref[0], bits=False)
        else:
            chk.within(tag + "dpre", dpre_got, dpre_ref[0], dpre_ref[1])


MUTANTS = ("last_max", "grad_at_zero", "unflipped", "no_b2", "pad_ring", "one_minus_a", "drop_last_sample",
           "tail_column")


def mutant_run(c, name: str, rows: int = 2):
    """What a kernel with the named defect would hand the comparison functions on data set c (a QSC lattice case):
    NS(p1, c1, p2, c2 -- the forward state --, slab (rows, row) fp32, dpre, lay, bk: the TRUE backward oracle given
    that state, r: the true forward).  name = "": the unmutated oracle."""
    net, P = c.net, c.P
    assert net.name == "qsc"
    lay = qsc_layout(c.n, c.F)
    r = forward(net, c.x, P)
    p1, c1 = pool(r.z1, True, last=(name == "last_max"))
    p2, c2 = pool(r.z2, True, last=(name == "last_max"))
    d_true = dpre(c.angles, c.dang)
    d_mut = dpre(c.angles, c.dang, "one_minus_a" if name == "one_minus_a" else "")
    bk_true = backward(net, c.x, P, p1, c1, p2, c2, d_true[0], d_true[1])
    bk = backward(net, c.x, P, p1, c1, p2, c2, d_mut[0], mutant=name)
    slab = torch.zeros(rows, lay.row, dtype=torch.float32)
    slab[0] = row_of(lay, bk.g, torch.float32)
    if name == "tail_column":
        slab[rows - 1, int(gap_columns(lay, ("qw",)).nonzero()[-1])] = 2.0 ** -20
    return NS(p1=p1, c1=c1, p2=p2, c2=c2, slab=slab, dpre=d_mut[0], dpre_ref=d_true, lay=lay, bk=bk_true, r=r)
