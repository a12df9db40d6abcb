"""Float64 oracle of ONE update launch of the fused optimizers (csrc/hip/optim.hip adam_kernel / sgd_kernel, and the
EPI_ADAM epilogue of csrc/hip/gemm.hip) over a flat range: data generators, the reference, exactness conditions and
the derived error bounds.  Pure torch, any device; a helper module, not a conftest.  It models the operation from the
kernels' stated contract and does not read ops/optim.py's host path.

The operation, per stepped element (``Hyper`` holds the hyper-parameters AS THE KERNEL RECEIVES THEM: fp32 values --
f32(0.9), f32(1 - f32(0.9)), f32(1e-8), lr from the device's fp32 ``lr_t`` -- everything after that is float64;
``ideal=True`` keeps the float64 values exactly as given, the mode compared with torch.optim):

  gj = g * grad_scale
  prune when !(|gj| > prune_thr)  (prune_thr > 0; a NaN gradient is pruned): gj = 0, count += 1
  AdamW: p *= 1 - lr * wd              L2 (Adam, SGD): gj += wd * p, after pruning
  Adam:  t' = t + 1;  m = b1 m + (1 - b1) gj;  v = b2 v + (1 - b2) gj^2
         p -= lr / (1 - b1^t') * m / (sqrt(v) / sqrt(1 - b2^t') + eps)
  SGD:   buf = gj on the first step (t < 0.5), else momentum * buf + gj;  p -= lr * buf
  the gradient is stored back as the update used it (gj, L2 term included) when prune_thr > 0 or grad_scale != 1, and
  always for the elements of a slab job; any other launch leaves the gradient's bits alone.

Which elements are stepped:
  * ``hole`` = (hole_lo, hole_n): [hole_lo, hole_lo + hole_n) is another kernel's; p, m, v, g keep their bits.
  * slab jobs: job k's gradient over [off, off + groups * width) is out[g * width + i] = sum_r slab[(g * rows + r) *
    ld + i], summed here in float64.  The regular pass leaves the jobs' ranges out -- as SKIP INTERVALS: the ranges
    sorted and merged across gaps of fewer than 64 elements, and the elements of such a gap ARE NOT STEPPED AT ALL.
    That is the launcher's documented contract (a gap is alignment padding: zero gradient, never read), modelled
    here as it stands.  A gap that contains hole_lo is not merged.  ``skip_intervals`` raises ValueError where the
    launcher refuses: more than 4 intervals, overlapping jobs, a job touching the hole, width < 4, unaligned jobs.
  * ``skip`` (the NaN guard's flag): nothing changes, and the step counter does not tick.

Two kinds of data (``Case``):
  LATTICE  betas (0.5, 0.75); g, m, v and slab entries small integers over a power of two (|g| <= 64).  Every m, v,
           slab sum and written-back gradient is then an fp32 value whatever the order of operations, so the
           kernel's m, v, g and pruned count must equal the oracle's BIT FOR BIT (``Result.exact`` says whether the
           condition held; with L2 decay it holds for the first step only, p leaves the lattice).  prune_thr = 0.1 is
           off the lattice and grad_scale is 1 or 0.5: no prune decision depends on a rounding.
  REAL     randn-scaled, default betas; per-element bounds (``Result.bm / bv / bp``), derived at ``adam_bounds``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from conv_oracle import EPS_F32, SENTINEL, assert_equal, is_f32, round_bf16, worst_ratio  # noqa: F401 (re-exported)

D = torch.float64
U = EPS_F32            # unit roundoff of fp32, 2^-24
K_E = 8.0              # adam_elem's own roundings in the update (derived at adam_bounds)
K_S = 4.0              # __powf / rsqrtf (measured: docs/PARITY.md "optimizer oracle")
E4M3_MAX = 448.0
GAP = 64               # jobs closer than this are merged into one skip interval
MAX_SKIPS = 4
MAX_JOBS = 16


def f32(x: float) -> float:
    """The fp32 value the kernel receives for a host double."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32).to(D))


@dataclass
class Hyper:
    kind: str = "adam"                 # adam | adamw | sgd
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    wd: float = 0.0
    grad_scale: float = 1.0
    prune_thr: float = 0.0
    momentum: float = 0.9
    ideal: bool = False                # float64 hyper-parameters exactly as given

    def __post_init__(self):
        assert self.kind in ("adam", "adamw", "sgd")
        r = (lambda x: float(x)) if self.ideal else f32
        self.b1, self.b2 = r(self.betas[0]), r(self.betas[1])
        # (the kernel forms 1.f - beta in fp32)
        self.omb1, self.omb2 = r(1.0 - self.b1), r(1.0 - self.b2)
        self.eps_, self.wd_, self.gs, self.thr, self.mom = r(self.eps), r(self.wd), r(self.grad_scale), \
            r(self.prune_thr), r(self.momentum)
        self.decoupled = self.kind == "adamw"
        self.writes_grad = self.thr > 0 or self.gs != 1.0


@dataclass
class Job:
    """One slab job: slab (groups * rows, ld) float, gradient of [off, off + groups * width)."""
    off: int
    groups: int
    rows: int
    width: int
    ld: int
    slab: torch.Tensor

    @property
    def hi(self) -> int:
        return self.off + self.groups * self.width

    def sums(self, absolute: bool = False) -> torch.Tensor:
        s = self.slab.to(D).reshape(self.groups, self.rows, self.ld)[:, :, :self.width]
        return (s.abs() if absolute else s).sum(1).reshape(-1)


def skip_intervals(jobs: Sequence[Job], n: int, hole: Tuple[int, int] = (0, 0)) -> List[Tuple[int, int]]:
    """The launcher's skip intervals of the regular pass; ValueError where the launcher refuses the launch."""
    hole_lo, hole_n = hole
    if len(jobs) > MAX_JOBS:
        raise ValueError("too many jobs")
    for j in jobs:
        if j.off < 0 or j.groups < 1 or j.rows < 1 or j.width < 4 or j.ld < j.width or (j.off | j.width | j.ld) & 3 \
                or j.hi > n:
            raise ValueError(f"bad job {j.off, j.groups, j.rows, j.width, j.ld}")
        if hole_n and j.off < hole_lo + hole_n and hole_lo < j.hi:
            raise ValueError("job inside the hole")
    out: List[List[int]] = []
    prev_hi = None
    for j in sorted(jobs, key=lambda j: j.off):
        if prev_hi is not None and j.off < prev_hi:
            raise ValueError("overlapping jobs")
        prev_hi = j.hi
        if out and j.off - out[-1][1] < GAP and not (hole_n and out[-1][1] <= hole_lo < j.off):
            out[-1][1] = j.hi
        else:
            if len(out) == MAX_SKIPS:
                raise ValueError("more than 4 skip intervals")
            out.append([j.off, j.hi])
    return [(a, b) for a, b in out]


def slab_model(jobs: Sequence[Job], n: int, hole: Tuple[int, int] = (0, 0), device=None):
    """(gsum, in_job, skipped, dsum): the jobs' float64 gradients scattered over n elements, the elements a job owns,
    the elements the regular pass leaves out (the skip intervals: the jobs' and the merged gaps'), and the bound of
    an fp32 sum of the rows in any order, rows * u * sum |x| (conv_oracle.sum_bound)."""
    gsum = torch.zeros(n, dtype=D, device=device)
    dsum = torch.zeros(n, dtype=D, device=device)
    in_job = torch.zeros(n, dtype=torch.bool, device=device)
    skipped = torch.zeros(n, dtype=torch.bool, device=device)
    for a, b in skip_intervals(jobs, n, hole):
        skipped[a:b] = True
    for j in jobs:
        gsum[j.off:j.hi] = j.sums().to(gsum.device)
        dsum[j.off:j.hi] = j.rows * U * j.sums(absolute=True).to(gsum.device)
        in_job[j.off:j.hi] = True
    return gsum, in_job, skipped, dsum


@dataclass
class Result:
    p: torch.Tensor
    m: torch.Tensor                    # (SGD: the momentum buffer)
    v: Optional[torch.Tensor]
    g: torch.Tensor                    # the gradient buffer after the launch
    pruned: int
    t: float
    stepped: torch.Tensor              # bool: the elements this launch updated
    exact: bool                        # every m, v, g is an fp32 value (the lattice's condition)
    bp: torch.Tensor = None            # REAL bounds (zero where nothing was stepped)
    bm: torch.Tensor = None
    bv: torch.Tensor = None
    bg: torch.Tensor = None            # bound of the stored gradient (zero where the launch leaves it alone)
    ambiguous: int = 0                 # prune decisions within 4u thr of the threshold
    shadow: Optional[torch.Tensor] = None     # round_bf16(p) over the shadow range
    e4m3: Optional[torch.Tensor] = None       # uint8 bytes of e4m3(clamp(p * qs)) over the shadow range
    wmax: float = 0.0                         # max |p| over the shadow range
    terms: dict = field(default_factory=dict)


def e4m3_bytes(x: torch.Tensor) -> torch.Tensor:
    """float64 -> fp32 -> clamp(+-448) -> torch's e4m3 cast, as bytes."""
    return x.to(torch.float32).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def shadows(p: torch.Tensor, rng: Tuple[int, int], qs: Optional[float] = None):
    """(bf16 shadow as float64, e4m3 bytes or None, max |p|) of p[lo:hi] -- ``p`` an fp32-valued tensor."""
    w = p[rng[0]:rng[1]].to(D)
    # (the rounding itself on the CPU: conv_oracle.round_bf16 builds on frexp / ldexp, whose float64 device versions
    # are not what the conv oracle was checked with)
    return round_bf16(w.cpu()).to(w.device), (e4m3_bytes(w * qs) if qs is not None else None), \
        (float(w.abs().max()) if w.numel() else 0.0)


def step(hp: Hyper, p, g, m, v, t: float, lr: float, hole: Tuple[int, int] = (0, 0), jobs: Sequence[Job] = (),
         shadow: Optional[Tuple[int, int]] = None, qs: Optional[float] = None, skip: bool = False) -> Result:
    """One launch over the flat range (p, g, m, v of n elements; SGD: m = buf, v = None) at step count ``t`` (the
    value of the device counter BEFORE the launch) and learning rate ``lr``."""
    p, g, m = p.to(D), g.to(D), m.to(D)
    v = v.to(D) if v is not None else None
    n, dev = p.numel(), p.device
    zeros = torch.zeros(n, dtype=D, device=dev)
    if skip:
        none = torch.zeros(n, dtype=torch.bool, device=dev)
        return Result(p, m, v, g, 0, t, none, True, zeros, zeros, zeros, zeros)
    gsum, in_job, skipped, dsum = slab_model(jobs, n, hole, dev)
    stepped = ~skipped | in_job
    stepped[hole[0]:hole[0] + hole[1]] = False
    g_in = torch.where(in_job, gsum, g)
    gs = g_in * hp.gs
    keep = gs.abs() > hp.thr if hp.thr > 0 else torch.ones(n, dtype=torch.bool, device=dev)
    pruned = int((~keep & stepped).sum())
    amb = int((((gs.abs() - hp.thr).abs() <= 4 * U * hp.thr + dsum * hp.gs) & stepped).sum()) if hp.thr > 0 else 0
    gj = torch.where(keep, gs, zeros)
    p0 = p * (1.0 - lr * hp.wd_) if hp.decoupled else p
    if not hp.decoupled and hp.wd_ != 0.0:
        gj = gj + hp.wd_ * p
    # error already in gj when the moments consume it: the scale's product, the L2 term's product and sum
    dg = torch.where(keep, U * gs.abs() * float(hp.gs != 1.0) + dsum * abs(hp.gs), zeros)
    if not hp.decoupled and hp.wd_ != 0.0:
        dg = dg + 2 * U * (gj - hp.wd_ * p).abs() + 2 * U * (hp.wd_ * p).abs()
    terms = {}
    if hp.kind == "sgd":
        b = gj if t < 0.5 else hp.mom * m + gj
        pn = p0 - lr * b
        bm = dg if t < 0.5 else 2 * U * ((hp.mom * m).abs() + gj.abs()) + dg
        bp = U * pn.abs() + 2 * U * (lr * b).abs() + lr * bm
        mn, vn, bv = b, None, zeros
    else:
        tt = t + 1.0
        mn = hp.b1 * m + hp.omb1 * gj
        vn = hp.b2 * v + hp.omb2 * gj * gj
        mn, vn, pn, bm, bv, bp, terms = adam_bounds(hp, p0, m, v, gj, mn, vn, tt, lr, dg)
        if hp.decoupled:   # the factor 1 - lr wd and the product, one rounding each
            bp = bp + 2 * U * p0.abs()
    sel = lambda new, old: torch.where(stepped, new, old)
    wb = (stepped & in_job) | (stepped if hp.writes_grad else torch.zeros_like(stepped))
    res = Result(sel(pn, p), sel(mn, m), sel(vn, v) if v is not None else None, torch.where(wb, gj, g), pruned,
                 t + 1.0, stepped, False, sel(bp, zeros), sel(bm, zeros), sel(bv, zeros),
                 torch.where(wb, dg, zeros), amb, terms=terms)
    res.exact = is_f32(res.m) and is_f32(res.g) and (res.v is None or is_f32(res.v)) and is_f32(gs)
    if shadow is not None:
        res.shadow, res.e4m3, res.wmax = shadows(res.p, shadow, qs)
    return res


def adam_bounds(hp: Hyper, p0, m, v, gj, mn, vn, tt: float, lr: float, dg):
    """The float64 Adam update and the bounds of its fp32 evaluation (common.h adam_elem), u = 2^-24:

      m' = fma(b1, m, fl((1 - b1) g)): the product's rounding and the fma's, each at most u times the larger of the
           result and its addends -- |dm| <= 3u (|b1 m| + |(1 - b1) g|), plus (1 - b1) times the error already in g.
      v' = fma(b2, v, fl(fl((1 - b2) g) g)): one rounding more -- |dv| <= 4u (|b2 v| + (1 - b2) g^2), plus
           2 (1 - b2) |g| times the error in g.
      p' = fma(-step_size, fl(m' / denom), p), denom = fma(sqrt(v'), rbc2, eps), step_size = fl(lr / bc1):
           u |p'| for the last rounding; the update upd = step_size m' / denom carries the relative errors of the
           square root, the two fmas, the divide and step_size's own divide and 1 - b1^t subtraction, K_E = 8
           roundings in all with room for second-order terms; bc1 = 1 - b1^t and bc2 = 1 - b2^t carry __powf's error
           amplified by b^t / (1 - b^t) (bc2 enters through a square root: the factor 0.5) and rsqrtf's own, K_S
           roundings of the intrinsics (measured, not derived); and the moments' errors pass through
           d upd / dm = step_size / denom and d upd / dv = upd * rbc2 / (2 sqrt(v') denom)."""
    b1t, b2t = hp.b1 ** tt, hp.b2 ** tt
    bc1, bc2 = 1.0 - b1t, 1.0 - b2t
    step_size, rbc2 = lr / bc1, bc2 ** -0.5
    sq = vn.sqrt()
    denom = sq * rbc2 + hp.eps_
    upd = step_size * mn / denom
    pn = p0 - upd
    bm = 3 * U * ((hp.b1 * m).abs() + (hp.omb1 * gj).abs()) + hp.omb1 * dg
    bv = 4 * U * ((hp.b2 * v).abs() + hp.omb2 * gj * gj) + 2 * hp.omb2 * gj.abs() * dg
    amp = b1t / bc1 + 0.5 * b2t / bc2
    t_e = upd.abs() * K_E * U
    t_s = upd.abs() * K_S * U * amp
    t_m = step_size / denom * bm
    dudv = torch.where(sq > 0, upd.abs() * rbc2 / (2 * sq.clamp_min(1e-300) * denom), torch.zeros_like(upd))
    t_v = dudv * bv
    bp = U * pn.abs() + t_e + t_s + t_m + t_v
    return mn, vn, pn, bm, bv, bp, dict(upd=upd, t_e=t_e, t_s=t_s, t_m=t_m, t_v=t_v, amp=amp)


# ------------------------------------------------------------------------------------------ data
LATTICE_BETAS = (0.5, 0.75)


class Case:
    """The operands of one (mode, n, seed): p, m, v (and buf = m) before the first step and ``steps`` gradients,
    generated once on the CPU as fp32-valued float64 tensors and cached."""

    def __init__(self, mode: str, n: int, seed: int, steps: int = 3):
        assert mode in ("lattice", "real")
        self.mode, self.n, self.seed, self.steps = mode, n, seed, steps
        gen = torch.Generator().manual_seed(7919 * seed + n)
        if mode == "lattice":
            ri = lambda lo, hi: torch.randint(lo, hi + 1, (n,), generator=gen).to(D)
            self.p = ri(-16, 16) / 8
            self.m = ri(-8, 8) / 2
            self.v = ri(0, 16) / 4
            # one gradient in eight is zero (pruned); the others are at least 1/2 in magnitude
            self.g = [torch.where(ri(0, 7) == 0, torch.zeros(n, dtype=D), ri(-128, 128) / 2) for _ in range(steps)]
            self.betas = LATTICE_BETAS
        else:
            rn = lambda s: (s * torch.randn(n, generator=gen)).to(D)   # (fp32 randn: fp32 values)
            self.p, self.m = rn(1.0), rn(0.1)
            self.v = (rn(0.1) ** 2).to(torch.float32).to(D)
            self.g = [rn(0.3) for _ in range(steps)]
            self.betas = (0.9, 0.999)

    def slab(self, groups: int, rows: int, ld: int, k: int = 0) -> torch.Tensor:
        """A (groups * rows, ld) slab of this case's kind (job ``k`` of the case)."""
        gen = torch.Generator().manual_seed(104729 * self.seed + 31 * k + rows + 7 * ld)
        if self.mode == "lattice":
            return torch.randint(-8, 9, (groups * rows, ld), generator=gen).to(D) / 2
        return (0.3 / rows ** 0.5 * torch.randn(groups * rows, ld, generator=gen)).to(D)


# REAL seeds: chosen so that no prune decision of any step and scale is ambiguous (asserted by
# tests/test_optim_oracle_cpu.py); sizes not listed use seed 0
REAL_SEEDS = {2 ** 20 - 16: 1}


@functools.lru_cache(maxsize=None)
def case(mode: str, n: int, steps: int = 3) -> Case:
    return Case(mode, n, REAL_SEEDS.get(n, 0) if mode == "real" else 0, steps)


# ------------------------------------------------------------------------------------------ shared test tables
# the plain-update sizes of tests/test_optim_exact_gpu.py (n, max_grid): one workgroup with 4 live threads; four
# workgroups, the last nearly empty; grid-stride rounds with a partial last one; either side of the 2^20 switch to
# non-temporal accesses
SIZES = ((16, 0), (3 * 1024 + 16, 0), (6 * 1024 + 48, 2), (2 ** 20 - 16, 0), (2 ** 20 - 16, 64), (2 ** 20 + 16, 0),
         (2 ** 20 + 16, 64))
SCALES = (1.0, 0.5, 1.0 / 3.0)
PRUNE_THR = 0.1

# slab-job layouts: name -> (n, hole, ((off, groups, rows, width, ld), ...)).  rows 1 .. 130 walk the kernel's 16 row
# phases in rounds of 4 (a partial phase, one round, one round + 1, several rounds); widths below, at and above the
# 64 columns of a workgroup; padded and dense rows; one and several groups.
SLAB_LAYOUTS = {
    # adjacent jobs, a 16-element gap (merged: [248, 264) is not stepped), a 64-element gap that is a real parameter
    # ([328, 392): stepped by the regular pass), a far job: 3 skip intervals
    "mixed": (8192, (0, 0), ((64, 1, 1, 4, 4), (68, 3, 15, 60, 72), (264, 1, 16, 64, 64), (392, 1, 17, 68, 80),
                             (460, 3, 64, 2048, 2048), (6604, 1, 65, 64, 76), (7168, 1, 130, 4, 16))),
    # a 48-element gap [192, 240) that contains the hole [208, 224): not merged, its other 32 elements are stepped
    "hole": (4096, (208, 16), ((128, 1, 17, 64, 76), (240, 3, 15, 60, 60), (2048, 1, 64, 68, 68))),
}
SLAB_REFUSALS = {
    "five intervals": (4096, (0, 0), tuple((512 * k, 1, 2, 64, 64) for k in range(5))),
    "overlap": (4096, (0, 0), ((64, 1, 2, 64, 64), (96, 1, 2, 64, 64))),
    "job in hole": (4096, (1024, 256), ((1152, 1, 2, 64, 64),)),
    "width 2": (4096, (0, 0), ((64, 1, 2, 2, 4),)),
}


def layout_jobs(cs: Case, specs, device=None) -> List[Job]:
    """The Jobs of a layout with this case's kind of slab data (fp32 slabs on ``device``)."""
    return [Job(off, groups, rows, width, ld, cs.slab(groups, rows, ld, k).to(torch.float32).to(device))
            for k, (off, groups, rows, width, ld) in enumerate(specs)]
