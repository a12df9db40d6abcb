"""The scenario classifier kernels (csrc/hip/sc.hip, qsc.hip, qsc_mfma.hip) against the float64 oracle of
tests/classifier_oracle.py, through the native entry points with synthetic flat buffers and hand-made ``offs``.

LATTICE data: every comparison is an equality (torch.equal on the values, on the bit patterns where a signed zero
matters).  REAL data: every comparison is per element against a bound the oracle derives from the sums of absolute
addends; a pool choice that differs from float64's passes only as a near-tie.  Every output buffer is prefilled with
NaN (integer buffers with a sentinel) and must be written whole.  Each bounded comparison prints its achieved
max(err / bound) as ``ERRBOUND <what> <case> <ratio>`` (profiles/classifier_oracle_bounds.txt holds the table).
"""
import ctypes

import pytest
import torch

import classifier_oracle as co
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat

pytestmark = pytest.mark.gpu
_p, _i = ctypes.c_void_p, ctypes.c_int
D, F32 = torch.float64, torch.float32
INVALID = 1   # hipErrorInvalidValue
NAN = float("nan")


def P(t):
    return nat.ptr(t) if t is not None else None


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def nanbuf(dev, *shape):
    return torch.full(shape, NAN, device=dev, dtype=F32)


def sent(dev, dtype, *shape):
    return torch.full(shape, 0x55 if dtype == torch.uint8 else 0x55555555, device=dev, dtype=dtype)


def written(chk, what, t):
    chk.true(not bool(torch.isnan(t).any()), f"{what}: elements left unwritten (NaN)")


def untouched(t):
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == sent(t.device, t.dtype, 1)).all())


@pytest.fixture(scope="module")
def L(cuda):
    lib = nat.hip_lib()
    f = lambda name, args: nat.fn(lib, name, args)
    return dict(
        fwd=f("qd_qsc2_fwd", [_p] * 8 + [_i] * 5 + [_p]), fwd3=f("qd_qsc2_fwd3", [_p] * 8 + [_i] * 5 + [_p, _p]),
        bwd=f("qd_qsc2_bwd", [_p] * 12 + [_i] * 7 + [_p]), bwd3=f("qd_qsc2_bwd3", [_p] * 12 + [_i] * 7 + [_p, _p]),
        wlk=f("qd_qsc2_wl_in_kernel", [_i, _i, _i]), waves=f("qd_qsc2_waves", [_i, _i]),
        pre_fwd=f("qd_qsc_pre_fwd", [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
        pre_bwd=f("qd_qsc_pre_bwd", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
        head=f("qd_qsc_head", [_p] * 10 + [_i] * 5 + [_p]), ihead=f("qd_qsc_infer_head", [_p] * 5 + [_i] * 3 + [_p]),
        outer=f("qd_outer_partial", [_p, _p, _p, _i, _i, _i, _i, _p]),
        sc_fwd=f("qd_sc_fwd", [_p, _p, _p, _p, _i, _i, _i, _i] + [_p] * 9),
        sc_bwd=f("qd_sc_bwd", [_p, _p, _p, _i, _i, _i, _i] + [_p] * 7),
        sc_fin=f("qd_sc_finish", [_p, _i, _i, _p, _p, _p, _i, _p]))


def grids(waves):
    """(B, grid): one sample; an idle wave beside a partly filled last workgroup; unequal sample counts per wave under
    the grid-stride loop (one and two workgroups); workgroups with no sample at all."""
    return ((1, 1), (waves + 1, 2), (3 * waves + 1, 1), (2 * waves + 3, 2), (5, 5))


# ================================================================================ MFMA preprocess
class Q2:
    """One data set on the device and the four qsc_mfma.hip entry points on it."""

    def __init__(self, L, dev, c, lay=None, fill=0.0):
        self.L, self.dev, self.c = L, dev, c
        self.lay = lay or co.qsc_layout(c.n, c.F)
        self.flat = co.pack(self.lay, c.P, fill).to(dev)
        self.offs = ints(*self.lay.offs)
        self.x = c.x.to(F32).to(dev).contiguous()
        self.hw2 = c.H * c.W // 4

    def forward(self, grid, x3, img=None, B=None, n=None, H=None, W=None):
        c, dev = self.c, self.dev
        Bb = c.B
        s = co.NS(angles=nanbuf(dev, Bb, c.n), p2=nanbuf(dev, Bb, c.F), p1s=nanbuf(dev, Bb, self.hw2, 16),
                  c1=sent(dev, torch.int32, Bb, self.hw2), c2=sent(dev, torch.uint8, Bb, c.F))
        args = [P(self.x), P(self.flat), self.offs, P(s.angles), P(s.p2), P(s.p1s), P(s.c1), P(s.c2),
                c.B if B is None else B, c.n if n is None else n, c.H if H is None else H, c.W if W is None else W, grid]
        st = nat.stream_ptr(dev)
        s.rc = self.L["fwd3"](*args, P(img), st) if x3 else self.L["fwd"](*args, st)
        torch.cuda.synchronize()
        return s

    def backward(self, s, angles, dang, grid, x3, img=None, qslab=None, qrows=0, qwidth=0, B=None, n=None, H=None,
                 W=None):
        c, dev = self.c, self.dev
        o = co.NS(dpre=nanbuf(dev, c.B, c.n), slab=nanbuf(dev, max(grid, 1), self.lay.row))
        args = [P(self.x), P(self.flat), self.offs, P(angles), P(dang), P(o.dpre), P(o.slab), P(s.p2), P(s.p1s), P(s.c1),
                P(s.c2), P(qslab), qrows, qwidth, c.B if B is None else B, c.n if n is None else n,
                c.H if H is None else H, c.W if W is None else W, grid]
        st = nat.stream_ptr(dev)
        o.rc = self.L["bwd3"](*args, P(img), st) if x3 else self.L["bwd"](*args, st)
        torch.cuda.synchronize()
        return o

    def state(self, s):
        """The saved buffers decoded to the oracle's (B, C, h, w) tensors (float64 / int64, on the CPU)."""
        c = self.c
        h, w = c.H // 2, c.W // 2
        return (co.dec_p1s(s.p1s.cpu().to(D), h, w), co.dec_c1(s.c1.cpu(), h, w),
                s.p2.cpu().to(D).view(c.B, 32, h // 2, w // 2), co.dec_u8(s.c2.cpu(), 32, h // 2, w // 2))


def _img(dev):
    return torch.zeros(2 * 9 * 16 * 48, device=dev, dtype=torch.bfloat16)


def check_q2_forward(chk, q, s, x3, tag):
    c = q.c
    lattice = c.mode == "lattice"
    chk.true(s.rc == 0, f"{tag} status {s.rc}")
    for k in ("angles", "p2", "p1s"):
        written(chk, tag + k, getattr(s, k))
    p1, c1, p2, c2 = q.state(s)
    chk.true(bool((s.c2 <= 3).all()), tag + "c2 codes 0..3, all written")
    dep = co.linear_depth("qsc2", c.F)
    r = co.forward(c.net, c.x, c.P, x3=x3, depth3=dep) if lattice else \
        co.forward(c.net, c.x, c.P, p1=p1, p2=p2, x3=x3, depth3=dep)
    co.check_forward_state(chk, c.net, lattice, r, p1, c1, p2, c2, tag)
    if lattice:   # the encodings themselves, bit for bit
        chk.equal(tag + "p1s", s.p1s, co.enc_p1s(r.p1), bits=True)
        chk.equal(tag + "c1 words", s.c1, co.enc_c1(r.c1))
        chk.equal(tag + "c2 bytes", s.c2, co.enc_u8(r.c2))
        chk.equal(tag + "p2", s.p2, r.p2.flatten(1), bits=True)
    chk.within(tag + "angles", s.angles, torch.tanh(r.z3), co.tanh_bound(r.z3, 0.0 * r.b3 if lattice else r.b3))
    return r


def check_q2_backward(chk, q, s, o, angles, dang, grid, waves, x3, wlk, tag, extra=None):
    c = q.c
    lattice = c.mode == "lattice"
    chk.true(o.rc == 0, f"{tag} status {o.rc}")
    written(chk, tag + "dpre", o.dpre)
    p1, c1, p2, c2 = q.state(s)
    d = co.dpre(angles.cpu(), dang.cpu())
    bk = co.backward(c.net, c.x, c.P, p1, c1, p2, c2, d[0], None if lattice else d[1], x3=x3)
    absent = () if wlk else ("wl",)
    co.check_backward(chk, q.lay, lattice, bk, o.slab, absent, o.dpre, d, tag, extra)
    slab = o.slab.cpu()
    for wg in range(grid):            # a workgroup without a sample: zeros apart from its quantum share
        if wg * waves >= c.B:
            row = slab[wg].clone()
            if extra:
                a, n_ = q.lay.ranges["qw"]
                row[a - q.lay.base:a - q.lay.base + n_] = 0
            chk.equal(f"{tag}sample-less workgroup {wg}", row, torch.zeros_like(row), bits=True)
    return bk


@pytest.mark.parametrize("mode", ["lattice", "real"])
@pytest.mark.parametrize("n", [1, 4, 6, 8, 9, 16])
@pytest.mark.parametrize("pilot", [128, 256])
def test_qsc2_forward_and_backward(cuda, L, pilot, n, mode):
    """qd_qsc2_fwd / fwd3 / bwd / bwd3 (bwd3: P128) on every (B, grid) of ``grids``: saved maps, choice codes, angles,
    dpre and every slab column."""
    H, W = co.GEOS[pilot]
    wlk = L["wlk"](H, W, n)
    wf, wb = L["waves"](W, 0), L["waves"](W, 1)
    assert wf > 0 and wb > 0
    chk = co.Check(f"P{pilot} n{n} {mode}")
    cases = sorted(set(grids(wf)) | set(grids(wb)))
    for B, grid in cases:
        c = co.case("qsc", pilot, B, n, mode)
        q = Q2(L, cuda, c)
        img = _img(cuda)
        states = {}
        for x3 in (False, True):
            tag = f"B{B} g{grid} {'fwd3' if x3 else 'fwd'} "
            s = q.forward(grid, x3, img if (x3 and pilot == 128) else None)
            check_q2_forward(chk, q, s, x3, tag)
            states[x3] = s
        if (B, grid) not in grids(wb):
            continue
        s = states[False]
        if mode == "lattice":
            ang, dang = c.angles.to(F32).to(cuda), c.dang.to(F32).to(cuda)
        else:
            ang, dang = s.angles, c.dang.to(F32).to(cuda)
        o = q.backward(s, ang, dang, grid, False)
        check_q2_backward(chk, q, s, o, ang, dang, grid, wb, False, wlk, f"B{B} g{grid} bwd ")
        if pilot == 128:
            s3 = states[True]
            if mode == "real":
                ang = s3.angles
            o3 = q.backward(s3, ang, dang, grid, True, img)
            check_q2_backward(chk, q, s3, o3, ang, dang, grid, wb, True, wlk, f"B{B} g{grid} bwd3 ")
            o3n = q.backward(s3, ang, dang, grid, True, None)
            check_q2_backward(chk, q, s3, o3n, ang, dang, grid, wb, True, wlk, f"B{B} g{grid} bwd3 (null image) ")
            chk.equal(f"B{B} g{grid} bwd3 image vs null: slab", o3.slab, o3n.slab, bits=True)
            chk.equal(f"B{B} g{grid} bwd3 image vs null: dpre", o3.dpre, o3n.dpre, bits=True)
    assert {L["wlk"](H, W, k) for k in (1, 4, 6, 8, 9, 16)} == {0, 1}   # both answers occur at this geometry
    chk.done()


@pytest.mark.parametrize("kernel,pilot", [("bwd", 128), ("bwd3", 128), ("bwd", 256)])
def test_qsc2_backward_folds_the_quantum_slab(cuda, L, kernel, pilot):
    """The quantum layer's slab rows, summed by the backward's workgroups into the quantum-weight columns of their own
    slab rows: integer contents, exact column sums, for a share longer than the 16 prefetched rows, a width that is
    no multiple of 4, the 256 limit, and the quantum weights before and after the preprocess parameters."""
    n, B, grid = 4, 5, 3
    H, W = co.GEOS[pilot]
    x3 = kernel == "bwd3"
    wb = L["waves"](W, 1)
    c = co.case("qsc", pilot, B, n, "lattice")
    chk = co.Check(f"{kernel} P{pilot}")
    g = torch.Generator().manual_seed(7)
    for qwidth in (30, 36, 256):
        for q_first in (True, False):
            lay = co.qsc_layout(n, c.F, qwidth=qwidth, q_first=q_first, lead=16)
            q = Q2(L, cuda, c, lay)
            s = q.forward(2, x3)
            ang, dang = c.angles.to(F32).to(cuda), c.dang.to(F32).to(cuda)
            for qrows in (1, grid - 1, 17 * grid + 3):
                qs = torch.randint(-8, 9, (qrows, qwidth), generator=g).to(F32)
                tag = f"qw{qwidth} {'before' if q_first else 'after'} rows{qrows} "
                o = q.backward(s, ang, dang, grid, x3, None, qs.to(cuda), qrows, qwidth)
                check_q2_backward(chk, q, s, o, ang, dang, grid, wb, x3, L["wlk"](H, W, n), tag,
                                  extra={"qw": qs.to(D).sum(0)})
            o = q.backward(s, ang, dang, grid, x3, None, None, 5, qwidth)
            check_q2_backward(chk, q, s, o, ang, dang, grid, wb, x3, L["wlk"](H, W, n),
                              f"qw{qwidth} {'before' if q_first else 'after'} null slab ")
    chk.done()


def test_qsc2_refusals_leave_the_outputs_untouched(cuda, L):
    c = co.case("qsc", 128, 5, 4, "lattice")
    lay = co.qsc_layout(4, c.F, qwidth=36, q_first=True)
    q = Q2(L, cuda, c, lay)
    good = q.forward(2, False)
    assert good.rc == 0
    ang, dang = c.angles.to(F32).to(cuda), c.dang.to(F32).to(cuda)
    bad = (dict(n=0), dict(n=17), dict(B=0), dict(grid=0), dict(H=8, W=8), dict(H=16, W=4))
    for kw in bad:
        kw = dict(kw)
        grid = kw.pop("grid", 2)
        for x3 in (False, True):
            s = q.forward(grid, x3, **kw)
            assert s.rc == INVALID, (kw, grid, x3, s.rc)
            assert all(untouched(getattr(s, k)) for k in ("angles", "p2", "p1s", "c1", "c2")), (kw, x3)
            o = q.backward(good, ang, dang, grid, x3, **kw)
            assert o.rc == INVALID, (kw, grid, x3, o.rc)
            assert untouched(o.dpre) and untouched(o.slab), (kw, x3)
    o = q.backward(good, ang, dang, 2, True, H=16, W=16)      # (bwd3 is P128 only)
    assert o.rc == INVALID and untouched(o.slab)
    qs = torch.ones(3, 257, device=cuda)
    for qwidth in (0, 257):
        o = q.backward(good, ang, dang, 2, True, None, qs, 3, qwidth)
        assert o.rc == INVALID and untouched(o.dpre) and untouched(o.slab), qwidth


# ================================================================================ reference path (qsc.hip)
def recomputed_forward(pilot, B, n, mode):
    """Data set and float64 forward for a kernel that recomputes its forward and hands out the angles only (qsc.hip):
    (c, r, e_p1, e_p2, b3) with every stage's error carried into the next.  REAL: the first seed whose float64
    forward has no near-tie and no pooled value within its bound of zero -- a property of the data, found without
    the kernel: the recomputed choices and masks are then float64's."""
    for seed in range(16):
        c = co.case("qsc", pilot, B, n, mode, seed)
        r = co.forward(c.net, c.x, c.P, depth3=co.linear_depth("qsc", c.F))
        e_p1 = co.windows(r.b1).amax(-1)
        b2 = r.b2 + co.F.conv2d(e_p1, c.P["w2"].abs(), padding=1)
        e_p2 = co.windows(b2).amax(-1)
        b3 = r.b3 + e_p2.flatten(1) @ c.P["wl"].abs().T
        if mode == "lattice" or (co.near_ties(r.z1, r.b1, True) == 0 and co.near_ties(r.z2, b2, True) == 0):
            return c, r, e_p1, e_p2, b3
    raise AssertionError("no tie-free data set among 16 seeds")


@pytest.mark.parametrize("mode", ["lattice", "real"])
@pytest.mark.parametrize("n", [4, 9])
@pytest.mark.parametrize("pilot", [128, 256])
def test_qsc_reference_path(cuda, L, pilot, n, mode):
    """qd_qsc_pre_fwd / qd_qsc_pre_bwd (the backward recomputes its forward): angles and every slab column."""
    H, W = co.GEOS[pilot]
    chk = co.Check(f"ref P{pilot} n{n} {mode}")
    lattice = mode == "lattice"
    for B, grid in ((1, 1), (5, 2), (7, 7)):
        c, r, e_p1, e_p2, b3 = recomputed_forward(pilot, B, n, mode)
        lay = co.qsc_layout(n, c.F, lead=32)
        flat = co.pack(lay, c.P).to(cuda)
        x = c.x.to(F32).to(cuda).contiguous()
        offs = ints(*lay.offs)
        st = nat.stream_ptr(cuda)
        angles = nanbuf(cuda, B, n)
        tag = f"B{B} g{grid} "
        assert L["pre_fwd"](P(x), P(flat), offs, P(angles), B, n, H, W, grid, st) == 0
        written(chk, tag + "angles", angles)
        e_a = co.tanh_bound(r.z3, 0.0 * b3 if lattice else b3)
        chk.within(tag + "angles", angles, torch.tanh(r.z3), e_a)
        dang = c.dang.to(F32).to(cuda)
        slab = nanbuf(cuda, grid, lay.row)
        assert L["pre_bwd"](P(x), P(flat), offs, P(dang), P(slab), B, n, H, W, grid, st) == 0
        torch.cuda.synchronize()
        # The backward recomputes the angles (the same device code on the same values as the forward kernel, whose
        # output is therefore what it uses) and tanh is not exact, so no lattice survives it: on LATTICE data the
        # slab is held to the bound of the one inexact step, dpre = dang (1 - angles^2), carried through exact sums
        # -- the lattice still brings its ties, zeros and dead windows to the recomputed pool choices.
        a = angles.cpu().to(D) if lattice else torch.tanh(r.z3)
        d = co.dpre(a, c.dang)
        if lattice:
            bk = co.backward(c.net, c.x, c.P, r.p1, r.c1, r.p2, r.c2, d[0], d[1])
        else:
            e3 = d[1] + 2 * c.dang.abs() * a.abs() * e_a
            bk = co.backward(c.net, c.x, c.P, r.p1, r.c1, r.p2, r.c2, d[0], e3, e_p1=e_p1, e_p2=e_p2)
        co.check_backward(chk, lay, False, bk, slab, tag=tag)
    chk.done()


def test_qsc_reference_path_refusals(cuda, L):
    c = co.case("qsc", 128, 5, 4, "lattice")
    lay = co.qsc_layout(4, c.F)
    flat, x, offs = co.pack(lay, c.P).to(cuda), c.x.to(F32).to(cuda).contiguous(), ints(*lay.offs)
    dang = c.dang.to(F32).to(cuda)
    st = nat.stream_ptr(cuda)
    for B, n, H, W, grid in ((5, 0, 16, 8, 2), (5, 17, 16, 8, 2), (0, 4, 16, 8, 2), (5, 4, 16, 8, 0), (5, 4, 8, 8, 2)):
        angles, slab = nanbuf(cuda, 5, 17), nanbuf(cuda, 2, lay.row)
        assert L["pre_fwd"](P(x), P(flat), offs, P(angles), B, n, H, W, grid, st) == INVALID, (B, n, H, W, grid)
        assert L["pre_bwd"](P(x), P(flat), offs, P(dang), P(slab), B, n, H, W, grid, st) == INVALID, (B, n, H, W, grid)
        torch.cuda.synchronize()
        assert untouched(angles) and untouched(slab)


# ================================================================================ qd_outer_partial
@pytest.mark.parametrize("Fd", [256, 512])
@pytest.mark.parametrize("n", [1, 9, 16])
def test_outer_partial(cuda, L, n, Fd):
    chk = co.Check(f"outer n{n} F{Fd}")
    g = torch.Generator().manual_seed(n * 1000 + Fd)
    st = nat.stream_ptr(cuda)
    for B, bs in ((1, 36), (37, 36), (73, 36), (130, 100), (64, 64)):
        S = -(-B // bs)
        for mode in ("lattice", "real"):
            if mode == "lattice":
                Dm = torch.randint(-4, 5, (B, n), generator=g).to(F32)
                Pm = torch.randint(-9, 10, (B, Fd), generator=g).to(F32)
            else:
                Dm, Pm = torch.randn(B, n, generator=g), torch.randn(B, Fd, generator=g)
            slab = nanbuf(cuda, S, n, Fd)
            assert L["outer"](P(Dm.to(cuda)), P(Pm.to(cuda)), P(slab), B, n, Fd, bs, st) == 0
            torch.cuda.synchronize()
            ref, bd = co.outer_partial(Dm, Pm, bs)
            written(chk, f"B{B} bs{bs} slab", slab)
            if mode == "lattice":
                chk.equal(f"B{B} bs{bs} slab", slab, ref)
            else:
                chk.within("outer slab", slab, ref, bd)
    slab = nanbuf(cuda, 1, 17, Fd)
    Dm, Pm = torch.ones(4, 17, device=cuda), torch.ones(4, Fd, device=cuda)
    assert L["outer"](P(Dm), P(Pm), P(slab), 4, 17, Fd, 4, st) == INVALID
    assert L["outer"](P(Dm), P(Pm), P(slab), 4, 16, Fd, 0, st) == INVALID
    torch.cuda.synchronize()
    assert untouched(slab)
    chk.done()


# ================================================================================ heads
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("n", [2, 8, 16])
def test_heads(cuda, L, n, C):
    """qd_qsc_head and qd_qsc_infer_head: loss, dE, dWc, dbc, logp, pred per element; accumulate, skip, loss_acc."""
    chk = co.Check(f"head n{n} C{C}")
    g = torch.Generator().manual_seed(17 * n + C)
    st = nat.stream_ptr(cuda)
    dev = cuda
    for B in (1, 63, 1024, 1025):
        E = (torch.rand(B, n, generator=g) * 2 - 1).to(F32)
        wc, bc = (torch.randn(C, n, generator=g) * 0.7).to(F32), (torch.randn(C, generator=g) * 0.3).to(F32)
        y = torch.randint(0, C, (B,), generator=g)
        r = co.head(E, wc, bc, y, depth=2 + 6 + 16)   # (a thread's samples, wave_sum's levels, the 16 waves)
        Ed, wd, bd_, yd = E.to(dev), wc.to(dev), bc.to(dev), y.to(dev)
        for accumulate in (0, 1):
            for skip_add, with_acc in ((0, True), (1, False)):
                tag = f"B{B} acc{accumulate} sadd{skip_add} "
                dE = nanbuf(dev, B, n)
                g0w, g0b = torch.randn(C, n, generator=g), torch.randn(C, generator=g)
                dwc = g0w.to(dev) if accumulate else nanbuf(dev, C, n)
                dbc = g0b.to(dev) if accumulate else nanbuf(dev, C)
                loss = nanbuf(dev, 1)
                lacc = torch.full((1,), 2.5, device=dev) if with_acc else None
                skip = torch.full((1,), 3.0, device=dev)
                rc = L["head"](P(Ed), P(wd), P(bd_), P(yd), P(dE), P(dwc), P(dbc), P(loss), P(lacc), P(skip), skip_add,
                               accumulate, B, n, C, st)
                torch.cuda.synchronize()
                chk.true(rc == 0, f"{tag}status {rc}")
                for k, t in (("dE", dE), ("dWc", dwc), ("dbc", dbc), ("loss", loss)):
                    written(chk, tag + k, t)
                chk.within("head dE", dE, r.dE, r.b_dE)
                a = float(accumulate)
                chk.within("head dWc", dwc, r.dWc + a * g0w.to(D), r.b_dWc + a * co.EPS * (r.dWc + g0w.to(D)).abs())
                chk.within("head dbc", dbc, r.dbc + a * g0b.to(D), r.b_dbc + a * co.EPS * (r.dbc + g0b.to(D)).abs())
                chk.within("head loss", loss[0], r.loss, r.b_loss)
                if with_acc:
                    chk.equal(tag + "loss_acc", lacc, (torch.full((1,), 2.5) + loss.cpu()))
                chk.equal(tag + "skip", skip, torch.full((1,), 3.0 if skip_add else 0.0))
        # a NaN in E: the NaN guard sets (skip_add: increments) the flag
        En = Ed.clone()
        En[B // 2, n - 1] = NAN
        for skip_add in (0, 1):
            skip = torch.full((1,), 3.0, device=dev)
            dE, dwc, dbc, loss = nanbuf(dev, B, n), nanbuf(dev, C, n), nanbuf(dev, C), nanbuf(dev, 1)
            assert L["head"](P(En), P(wd), P(bd_), P(yd), P(dE), P(dwc), P(dbc), P(loss), None, P(skip), skip_add, 0, B,
                             n, C, st) == 0
            torch.cuda.synchronize()
            chk.equal(f"B{B} NaN skip sadd{skip_add}", skip, torch.full((1,), 4.0 if skip_add else 1.0))
            chk.true(bool(torch.isnan(loss).all()), f"B{B} NaN loss")
        # without a skip flag at all
        dE, dwc, dbc, loss = nanbuf(dev, B, n), nanbuf(dev, C, n), nanbuf(dev, C), nanbuf(dev, 1)
        assert L["head"](P(Ed), P(wd), P(bd_), P(yd), P(dE), P(dwc), P(dbc), P(loss), None, None, 0, 0, B, n, C, st) == 0
        torch.cuda.synchronize()
        chk.within("head loss", loss[0], r.loss, r.b_loss)
        # inference head: both outputs, then each alone (the other null)
        ri = co.head(E, wc, bc, None)
        logp, pred = nanbuf(dev, B, C), sent(dev, torch.int64, B)
        assert L["ihead"](P(Ed), P(wd), P(bd_), P(logp), P(pred), B, n, C, st) == 0
        lp1, pr1 = nanbuf(dev, B, C), sent(dev, torch.int64, B)
        assert L["ihead"](P(Ed), P(wd), P(bd_), P(lp1), None, B, n, C, st) == 0
        assert L["ihead"](P(Ed), P(wd), P(bd_), None, P(pr1), B, n, C, st) == 0
        torch.cuda.synchronize()
        written(chk, f"B{B} infer logp", logp)
        chk.within("infer logp", logp, ri.logp, ri.b_logp)
        chk.true(bool(((pred >= 0) & (pred < C)).all()), f"B{B} infer pred written, in range")
        chk.true(bool(co.argmax_ok(pred.cpu(), ri).all()), f"B{B} infer pred: differs from float64 beyond a near-tie")
        chk.equal(f"B{B} infer logp alone", lp1, logp, bits=True)
        chk.equal(f"B{B} infer pred alone", pr1, pred)
    for nn, CC, Bz in ((1, 3, 4), (17, 3, 4), (8, 5, 4), (n, C, 0)):   # (B = 0: the mean over no sample)
        dE, loss = nanbuf(dev, 4, max(nn, 1)), nanbuf(dev, 1)
        z = torch.zeros(64, device=dev)
        yy = torch.zeros(4, device=dev, dtype=torch.int64)
        assert L["head"](P(z), P(z), P(z), P(yy), P(dE), P(z), P(z), P(loss), None, None, 0, 0, Bz, nn, CC, st) == INVALID
        assert L["ihead"](P(z), P(z), P(z), P(dE), None, Bz, nn, CC, st) == INVALID
        torch.cuda.synchronize()
        assert untouched(dE) and untouched(loss)
    chk.done()


# ================================================================================ SC
class SCRun:
    def __init__(self, L, dev, c):
        self.L, self.dev, self.c = L, dev, c
        self.lay = co.sc_layout(c.F)
        self.flat = co.pack(self.lay, c.P).to(dev)
        self.offs = ints(*self.lay.offs)
        self.x = c.x.to(F32).to(dev).contiguous()
        self.y = c.labels.to(dev)

    def forward(self, spb, train=True, labels=True, part=True, dlogit=True, logp=True, pred=True, B=None, H=None,
                W=None):
        c, dev = self.c, self.dev
        hw2 = 32 * c.H * c.W // 4
        grid = -(-c.B // max(spb, 1))
        s = co.NS(p1s=nanbuf(dev, c.B, hw2) if train else None, c1s=sent(dev, torch.uint8, c.B, hw2) if train else None,
                  p2s=nanbuf(dev, c.B, c.F) if train else None, c2s=sent(dev, torch.uint8, c.B, c.F) if train else None,
                  dlogit=nanbuf(dev, c.B, 4) if dlogit else None, part=nanbuf(dev, grid, 2) if part else None,
                  logp=nanbuf(dev, c.B, 3) if logp else None, pred=sent(dev, torch.int64, c.B) if pred else None, grid=grid)
        s.rc = self.L["sc_fwd"](P(self.x), P(self.flat), self.offs, P(self.y) if labels else None,
                                c.B if B is None else B, spb, c.H if H is None else H, c.W if W is None else W,
                                P(s.p1s), P(s.c1s), P(s.p2s), P(s.c2s), P(s.dlogit), P(s.part), P(s.logp), P(s.pred),
                                nat.stream_ptr(dev))
        torch.cuda.synchronize()
        return s

    def backward(self, s, dlogit, spb, B=None, H=None, W=None):
        c, dev = self.c, self.dev
        slab = nanbuf(dev, -(-c.B // max(spb, 1)), self.lay.row)
        rc = self.L["sc_bwd"](P(self.x), P(self.flat), self.offs, c.B if B is None else B, spb, c.H if H is None else H,
                              c.W if W is None else W, P(s.p1s), P(s.c1s), P(s.p2s), P(s.c2s), P(dlogit), P(slab),
                              nat.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, slab

    def state(self, s):
        c = self.c
        h, w = c.H // 2, c.W // 2
        return (s.p1s.cpu().to(D).view(c.B, 32, h, w), co.dec_u8(s.c1s.cpu(), 32, h, w),
                s.p2s.cpu().to(D).view(c.B, 32, h // 2, w // 2), co.dec_u8(s.c2s.cpu(), 32, h // 2, w // 2))


@pytest.mark.parametrize("mode", ["lattice", "real"])
@pytest.mark.parametrize("pilot", [128, 256])
def test_sc_forward_finish_backward(cuda, L, pilot, mode):
    chk = co.Check(f"sc P{pilot} {mode}")
    lattice = mode == "lattice"
    for B, spb in ((1, 1), (2, 3), (7, 3), (9, 4)):
        c = co.case("sc", pilot, B, 3, mode)
        run = SCRun(L, cuda, c)
        tag = f"B{B} spb{spb} "
        s = run.forward(spb)
        chk.true(s.rc == 0, f"{tag}fwd status {s.rc}")
        for k in ("p1s", "p2s", "part", "logp"):
            written(chk, tag + k, getattr(s, k))
        written(chk, tag + "dlogit", s.dlogit[:, :3])
        chk.true(bool(torch.isnan(s.dlogit[:, 3]).all()), tag + "dlogit's pad column written")
        chk.true(bool((s.c1s <= 3).all()) and bool((s.c2s <= 3).all()), tag + "codes 0..3, all written")
        p1, c1, p2, c2 = run.state(s)
        dep = co.linear_depth("sc", c.F)
        r = co.forward(c.net, c.x, c.P, depth3=dep) if lattice else co.forward(c.net, c.x, c.P, p1=p1, p2=p2, depth3=dep)
        co.check_forward_state(chk, c.net, lattice, r, p1, c1, p2, c2, tag)
        h = co.softmax_head(r.z3, 0.0 * r.b3 if lattice else r.b3, c.labels, 1.0 / B)
        chk.within("sc logp", s.logp, h.logp, h.b_logp)
        chk.within("sc dlogit", s.dlogit[:, :3], h.dlogit, h.b_dlogit)
        pred = s.pred.cpu()
        chk.true(bool(((pred >= 0) & (pred < 3)).all()), tag + "pred written, in range")
        chk.true(bool(co.argmax_ok(pred, h).all()), tag + "pred differs from float64 beyond a near-tie")
        # finish: loss, correct count, loss_acc, skip (set / added)
        for skip_add in (0, 1):
            out, lacc, skip = nanbuf(cuda, 2), torch.full((1,), 1.5, device=cuda), torch.full((1,), 2.0, device=cuda)
            assert L["sc_fin"](P(s.part), s.grid, B, P(out), P(lacc), P(skip), skip_add, nat.stream_ptr(cuda)) == 0
            torch.cuda.synchronize()
            written(chk, tag + "out", out)
            bl = (h.b_nll.sum() + (B + 2) * co.EPS * h.nll.abs().sum()) / B
            chk.within("sc loss", out[0], h.nll.sum() / B, bl)
            chk.equal(tag + "correct", out[1], (pred == c.labels).sum().to(F32))
            chk.equal(tag + "loss_acc", lacc, torch.full((1,), 1.5) + out[0:1].cpu())
            chk.equal(tag + "skip", skip, torch.full((1,), 2.0 if skip_add else 0.0))
        # inference forward: every nullable argument null in turn; logp / pred as the training forward's, bit for bit
        for kw in (dict(), dict(labels=False, part=False, dlogit=False), dict(labels=False, part=False, dlogit=False,
                   pred=False), dict(labels=False, part=False, dlogit=False, logp=False), dict(part=False),
                   dict(dlogit=False), dict(part=False, dlogit=False, logp=False)):
            t = run.forward(spb, train=False, **kw)
            chk.true(t.rc == 0, f"{tag}inference {kw} status {t.rc}")
            if t.logp is not None:
                chk.equal(f"{tag}inference logp {kw}", t.logp, s.logp, bits=True)
            if t.pred is not None:
                chk.equal(f"{tag}inference pred {kw}", t.pred, s.pred)
            if t.dlogit is not None:
                chk.equal(f"{tag}inference dlogit {kw}", t.dlogit[:, :3], s.dlogit[:, :3], bits=True)
            if t.part is not None:
                chk.equal(f"{tag}inference part {kw}", t.part, s.part, bits=True)
        # backward from the kernel's saved state
        if lattice:
            dl = torch.full((B, 4), NAN)
            dl[:, :3] = c.dlogit.to(F32)
            d3, e3 = c.dlogit, None
        else:
            dl = s.dlogit.cpu()
            d3, e3 = dl[:, :3].to(D), None
        rc, slab = run.backward(s, dl.to(cuda), spb)
        chk.true(rc == 0, f"{tag}bwd status {rc}")
        bk = co.backward(c.net, c.x, c.P, p1, c1, p2, c2, d3, e3)
        co.check_backward(chk, run.lay, lattice, bk, slab, tag=tag)
    # refusals
    s = run.forward(0)
    assert s.rc == INVALID and untouched(s.logp) and untouched(s.p1s)
    for kw in (dict(B=0), dict(H=8, W=8), dict(H=16, W=4)):
        s = run.forward(4, **kw)
        assert s.rc == INVALID and untouched(s.logp) and untouched(s.p1s) and untouched(s.part), kw
        rc, slab = run.backward(s, s.dlogit, 4, **kw)
        assert rc == INVALID and untouched(slab), kw
    rc, slab = run.backward(s, s.dlogit, 0)
    assert rc == INVALID and untouched(slab)
    out, part = nanbuf(cuda, 2), torch.zeros(4, 2, device=cuda)
    for nblk, Bz in ((0, 4), (4, 0)):
        assert L["sc_fin"](P(part), nblk, Bz, P(out), None, None, 0, nat.stream_ptr(cuda)) == INVALID
    torch.cuda.synchronize()
    assert untouched(out)
    chk.done()


# ================================================================================ end to end
def _fill(space, lay_names, c):
    with torch.no_grad():
        for name, k in lay_names:
            o = dict(zip(space.names, space.offsets))[name]
            space.flat[o:o + c.P[k].numel()] = c.P[k].reshape(-1).to(F32).to(space.flat.device)


def check_step_grads(chk, sp, names, c, bk, g0, accumulate, rows):
    """The flat gradient's parameter ranges against the backward oracle.  accumulate: the reduction adds ``rows`` slab
    rows and the old content g0 in some order: rows more additions on partial sums of magnitude <= |g0| + S."""
    offs = dict(zip(sp.names, sp.offsets))
    for name, k in names:
        o, num = offs[name], c.P[k].numel()
        ref, bound = bk.g[k].reshape(-1), bk.bound[k].reshape(-1) + rows * co.EPS * bk.S[k].reshape(-1)
        if accumulate:
            old = g0[o:o + num].to(D)
            ref, bound = ref + old, bound + (rows + 1) * co.EPS * old.abs()
        chk.within("step d" + k, sp.grad[o:o + num], ref, bound)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pilot", [128, 256])
def test_sc_step_end_to_end(cuda, pilot, accumulate):
    """SCStepHIP at B = 9: the flat gradient after the step's own slab reduction, per element, given the step's
    saved state."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import SC_P128
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.sc import SCStepHIP
    B = 9
    c = co.case("sc", pilot, B, 3, "real")
    m = SC_P128(pilot).to(cuda)
    sp = FlatParamSpace(list(m.named_parameters()), cuda)
    names = (("conv1.weight", "w1"), ("conv2.weight", "w2"), ("FC.weight", "wl"), ("FC.bias", "bl"))
    _fill(sp, names, c)
    step = SCStepHIP(m, sp, B)
    g0 = torch.randn(sp.numel, generator=torch.Generator().manual_seed(1)).to(F32)
    sp.grad.copy_(g0 if accumulate else torch.full_like(g0, NAN))
    x, y = c.x.to(F32).to(cuda).contiguous(), c.labels.to(cuda)
    step(x, y, accumulate=accumulate)
    torch.cuda.synchronize()
    p1s, c1s, p2s, c2s, dl = step._buf(B)[:5]
    h, w = c.H // 2, c.W // 2
    st = (p1s.cpu().to(D).view(B, 32, h, w), co.dec_u8(c1s.cpu(), 32, h, w), p2s.cpu().to(D).view(B, 32, h // 2, w // 2),
          co.dec_u8(c2s.cpu(), 32, h // 2, w // 2))
    bk = co.backward(c.net, c.x, c.P, *st, dl.cpu()[:, :3].to(D))
    chk = co.Check(f"sc step P{pilot} acc{int(accumulate)}")
    check_step_grads(chk, sp, names, c, bk, g0, accumulate, step._buf(B)[8])
    chk.done()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("impl", ["mfma", "ref"])
@pytest.mark.parametrize("pilot", [128, 256])
def test_qsc_step_end_to_end(cuda, L, pilot, impl, accumulate):
    """QSCStepHIP (both impl) at B = 2 waves + 1: the preprocess gradients in the flat space after the step's own slab
    reduction (and, where the kernel leaves it out, its outer-product GEMM), per element, given the step's saved
    state: p1s, c1, c2, p2, angles, dang for "mfma"; for "ref", which saves the angles only and recomputes the rest,
    the float64 forward of tie-free data with its error carried."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.models.estimators import QSC_P128
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import FlatParamSpace
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.qsc import QSCStepHIP
    H, W = co.GEOS[pilot]
    for n in (4, 9):
        B = 2 * L["waves"](W, 1) + 1
        if impl == "ref":
            c, r, e_p1, e_p2, _ = recomputed_forward(pilot, B, n, "real")
        else:
            c = co.case("qsc", pilot, B, n, "real")
        torch.manual_seed(0)
        m = QSC_P128(n_qubits=n, use_quantumnat=False, use_gradient_pruning=False, pilot_num=pilot).to(cuda)
        sp = FlatParamSpace(list(m.named_parameters()), cuda)
        names = (("preprocess.0.weight", "w1"), ("preprocess.0.bias", "b1"), ("preprocess.3.weight", "w2"),
                 ("preprocess.3.bias", "b2"), ("preprocess.7.weight", "wl"), ("preprocess.7.bias", "bl"))
        _fill(sp, names, c)
        step = QSCStepHIP(m, sp, B, impl=impl)
        g0 = torch.randn(sp.numel, generator=torch.Generator().manual_seed(1)).to(F32)
        sp.grad.copy_(g0 if accumulate else torch.full_like(g0, NAN))
        x, y = c.x.to(F32).to(cuda).contiguous(), c.labels.to(cuda)
        step(x, y, accumulate=accumulate)
        torch.cuda.synchronize()
        h, w = H // 2, W // 2
        d = co.dpre(step.angles.cpu(), step.dang.cpu())
        if impl == "mfma":
            st = (co.dec_p1s(step.p1s.cpu().to(D).view(B, h * w, 16), h, w), co.dec_c1(step.c1.cpu(), h, w),
                  step.p2.cpu().to(D).view(B, 32, h // 2, w // 2), co.dec_u8(step.c2.cpu(), 32, h // 2, w // 2))
            bk = co.backward(c.net, c.x, c.P, *st, d[0], d[1], x3=step.bwd_x3)
            rows = step.preslab.shape[0] + (0 if step.wl_in_kernel else step.wlslab.shape[0])
        else:   # (the backward's recomputed angles are the forward kernel's: the same device code on the same values)
            bk = co.backward(c.net, c.x, c.P, r.p1, r.c1, r.p2, r.c2, d[0], d[1], e_p1=e_p1, e_p2=e_p2)
            rows = step.preslab.shape[0]
        chk = co.Check(f"qsc step {impl} P{pilot} n{n} acc{int(accumulate)}")
        check_step_grads(chk, sp, names, c, bk, g0, accumulate, rows)
        chk.done()
