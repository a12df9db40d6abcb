"""The update launches of csrc/hip/optim.hip (adam_kernel, sgd_kernel, fp8_scale_update_kernel) and the EPI_ADAM
epilogue of csrc/hip/gemm.hip against the float64 oracle of tests/optim_oracle.py, on a real MI355X.

Every step is compared with ONE oracle step from the kernel's own state before it, so the bounds are single-step
bounds.  LATTICE data: the kernel's m, v, stored gradient and pruned count equal the oracle's bit for bit; REAL data:
every element of p, m, v and the stored gradient lies within the bounds derived in optim_oracle (no element is left
out; a bound of zero -- the hole, a merged gap, a sentinel, a gradient the launch leaves alone -- demands equal
bits).  Each case prints its worst error-to-bound ratios (``ORACLE ...`` lines, the table of docs/PARITY.md)."""
import ctypes

import pytest
import torch

import optim_oracle as oo
from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.fc import gemm_wgrad, gemm_wgrad_adam
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import (FP8_E4M3_MAX, FlatParamSpace,
                                                                                       Fp8Scales, FusedOptimizer)
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.slabsum import SlabBatch

pytestmark = pytest.mark.gpu
D = torch.float64
S = oo.SENTINEL
THR = oo.PRUNE_THR
# (kind, weight decay on REAL data, on LATTICE data): Adam, Adam with L2 decay, AdamW, SGD.  0.25 keeps g + wd p on
# the lattice for the first step (p leaves it then: the later steps are held to the bounds alone)
KINDS = {"adam": ("adam", 0.0, 0.0), "adam_l2": ("adam", 0.01, 0.25), "adamw": ("adamw", 0.01, 0.01),
         "sgd": ("sgd", 0.0, 0.0), "sgd_l2": ("sgd", 0.01, 0.25)}
MODES = ("lattice", "real")


# ------------------------------------------------------------------------------------------ helpers
def _opt(cuda, cs, kind, wd=0.0, prune=0.0, lr=1e-2, sizes=None, extra=0):
    """A FusedOptimizer over one space of cs.n elements (+ ``extra`` scratch) loaded with the case's p, m, v."""
    params = [torch.nn.Parameter(torch.zeros(s, device=cuda)) for s in (sizes or [cs.n])]
    space = FlatParamSpace([(f"p{i}", q) for i, q in enumerate(params)], cuda, extra=extra)
    assert space.extra_off == cs.n, (space.extra_off, cs.n)
    opt = FusedOptimizer(space, kind, lr=lr, betas=cs.betas, weight_decay=wd, prune_thr=prune,
                         momentum=0.5 if cs.mode == "lattice" else 0.9)
    space.flat[:cs.n].copy_(cs.p)
    if kind == "sgd":
        opt.buf[:cs.n].copy_(cs.m)
    else:
        opt.m[:cs.n].copy_(cs.m)
        opt.v[:cs.n].copy_(cs.v)
    return space, opt


def _hyper(cs, opt, scale=1.0):
    return oo.Hyper(opt.kind, betas=cs.betas, eps=opt.eps, wd=opt.weight_decay, grad_scale=scale,
                    prune_thr=opt.prune_thr, momentum=opt.momentum)


def _bufs(opt):
    s = opt.space
    return dict(p=s.flat, g=s.grad, m=opt.buf if opt.kind == "sgd" else opt.m, v=None if opt.kind == "sgd" else opt.v)


def _snap(opt):
    torch.cuda.synchronize()
    return {k: (x.clone() if x is not None else None) for k, x in _bufs(opt).items()}


def _unchanged(opt, before, lo=0, hi=None):
    torch.cuda.synchronize()
    for k, x in _bufs(opt).items():
        if x is not None:
            assert torch.equal(x[lo:hi], before[k][lo:hi]), f"{k}[{lo}:{hi}] changed"


def _compare(tag, mode, r, got, exact=True):
    """The kernel's range ``got`` (p, g, m, v) against the oracle Result; returns the worst ratios."""
    ratios = {}
    for k, ref, bound in (("p", r.p, r.bp), ("m", r.m, r.bm), ("v", r.v, r.bv), ("g", r.g, r.bg)):
        if ref is None:
            continue
        if mode == "lattice" and exact and k != "p":
            oo.assert_equal(f"{tag} {k}", got[k], ref)
        ratios[k] = oo.worst_ratio((got[k].to(D) - ref).abs(), bound)
    # (not a check of its own: the share of p's bound BEYOND its final rounding u |p| that the error beyond it uses,
    # i.e. how much of the K_E / K_S / moment terms the update needed)
    rnd = oo.U * r.p.abs()
    upd = oo.worst_ratio(((got["p"].to(D) - r.p).abs() - rnd).clamp_min(0), (r.bp - rnd).clamp_min(0) + 1e-300)
    print(f"ORACLE {tag} " + " ".join(f"{k}={x:.3f}" for k, x in ratios.items()) + f" upd={upd:.3f}")
    for k, x in ratios.items():
        assert x <= 1.0, f"{tag}: {k} is {x:.3f} times its bound"
    return ratios


def _step_and_check(tag, cs, opt, before, launch, lo, hi, slot, scale=1.0, exact=True, **kw):
    """Run ``launch()`` (one update launch over [lo, hi) with step slot ``slot``) and hold it to the oracle."""
    t, lr = float(opt.step_t[slot]), float(opt.lr_t)
    launch()
    torch.cuda.synchronize()
    sl = lambda x: x[lo:hi] if x is not None else None
    r = oo.step(_hyper(cs, opt, scale), sl(before["p"]), sl(before["g"]), sl(before["m"]), sl(before["v"]), t, lr, **kw)
    if cs.mode == "lattice":
        assert r.exact or not exact, f"{tag}: the lattice's exactness condition does not hold"
    assert r.ambiguous == 0, tag
    _compare(tag, cs.mode, r, {k: sl(x) for k, x in _bufs(opt).items()}, exact)
    assert float(opt.step_t[slot]) == r.t and int(opt.done[slot]) == 0, (tag, opt.step_t.tolist(), opt.done.tolist())
    return r


def _run_plain(cuda, tag, mode, n, kname, scale=1.0, prune=0.0, max_grid=0, steps=3, t0=0.0):
    kind, wd_real, wd_lat = KINDS[kname]
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, kind, wd_lat if mode == "lattice" else wd_real, prune)
    if max_grid:
        opt.max_grid[0] = max_grid
    opt.step_t.fill_(t0)
    total = 0
    for k in range(steps):
        space.grad.copy_(cs.g[k])
        before = _snap(opt)
        r = _step_and_check(f"{tag} {mode} {kname} n={n} t={t0 + k + 1:g}", cs, opt, before,
                            lambda: opt.step(grad_scale=scale), 0, n, 0, scale,
                            exact=not (kname.endswith("_l2") and k > 0))
        total += r.pruned
    assert int(opt.pruned) == total


# ------------------------------------------------------------------------------------------ sizes and paths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kname", ["adam", "adam_l2", "adamw", "sgd"])
@pytest.mark.parametrize("n,max_grid", oo.SIZES)
def test_sizes_and_paths(cuda, n, max_grid, kname, mode):
    """One workgroup, a nearly empty last workgroup, grid-stride rounds with a partial last one, and both sides of the
    2^20 switch to non-temporal accesses, capped and uncapped."""
    _run_plain(cuda, f"sizes grid={max_grid}", mode, n, kname, max_grid=max_grid)


@pytest.mark.parametrize("t0", [9, 999, 99999])
def test_large_step_count(cuda, t0):
    """step_t as a checkpoint load leaves it: the bias corrections b^t at t = 10, 1000, 100000."""
    _run_plain(cuda, "large-t", "real", 1040, "adam", steps=1, t0=float(t0))


# ------------------------------------------------------------------------------------------ direct launches
_ADAM_ARGS = [ctypes.c_void_p] * 4 + [ctypes.c_long] + [ctypes.c_void_p] * 4 + [ctypes.c_float] * 4 + \
    [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
     ctypes.c_int] + [ctypes.c_void_p] * 7


def _adam_raw(cuda, hp, p, g, m, v, n, lr_t, step_t, done, pruned, shadow=None, sh_lo=0, sh_hi=0):
    """qd_adam_step_slabs without the Python class (shapes FlatParamSpace never produces); returns the status."""
    f = nat.fn(nat.hip_lib(), "qd_adam_step_slabs", _ADAM_ARGS)
    return f(nat.ptr(p), nat.ptr(g), nat.ptr(m), nat.ptr(v), n, nat.ptr(lr_t), nat.ptr(step_t), None, nat.ptr(pruned),
             hp.betas[0], hp.betas[1], hp.eps, hp.wd, int(hp.decoupled), hp.grad_scale, hp.prune_thr, nat.ptr(done),
             nat.ptr(shadow) if shadow is not None else None, sh_lo, sh_hi, None, None, None, 0, None, 0, 0,
             0, None, None, None, None, None, None, nat.stream_ptr(cuda))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wd,scale,prune", [(0.0, 1.0, 0.0), (0.25, 1.0, 0.0), (0.0, 0.5, THR)])
def test_unaligned_tail(cuda, mode, wd, scale, prune):
    """n = 1027: the last 3 elements take the scalar tail path, with a bf16 shadow over [1020, 1028) that ends in it.
    Everything past n keeps its sentinel; a launch that neither scales nor prunes leaves the gradient's bits alone
    in the tail as in the vector path."""
    n, room = 1027, 1040
    cs = oo.case(mode, n)
    pad = lambda x: torch.cat([x.float(), torch.full((room - n,), S)]).to(cuda)
    p, m, v = pad(cs.p), pad(cs.m), pad(cs.v)
    lr_t, step_t = torch.full((1,), 1e-2, device=cuda), torch.zeros(1, device=cuda)
    done, pruned = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    shadow = torch.full((16,), S, device=cuda).bfloat16()
    hp = oo.Hyper("adam", betas=cs.betas, wd=wd, grad_scale=scale, prune_thr=prune)
    total = 0
    for k in range(3):
        g = pad(cs.g[k])
        before = [x.clone() for x in (p, g, m, v)]
        assert _adam_raw(cuda, hp, p, g, m, v, n, lr_t, step_t, done, pruned, shadow, 1020, 1028) == 0
        torch.cuda.synchronize()
        r = oo.step(hp, *[x[:n] for x in before], float(k), float(lr_t))
        assert r.ambiguous == 0
        _compare(f"tail {mode} wd={wd} scale={scale} t={k + 1}", mode, r, dict(p=p[:n], g=g[:n], m=m[:n], v=v[:n]),
                 exact=wd == 0 or k == 0)
        for x, b in zip((p, g, m, v), before):
            assert torch.equal(x[n:], b[n:])
        sh = oo.shadows(p, (1020, n))[0]
        assert torch.equal(shadow[:7].to(D), sh)
        assert bool((shadow[7:].float() == torch.tensor(S).bfloat16().float()).all())
        assert float(step_t) == k + 1 and int(done) == 0
        total += r.pruned
    assert int(pruned) == total


# ------------------------------------------------------------------------------------------ scale and pruning
@pytest.mark.parametrize("mode,scale", [("lattice", 0.5), ("real", 0.5), ("real", 1.0 / 3.0)])
@pytest.mark.parametrize("kname", ["adam", "adam_l2", "adamw", "sgd", "sgd_l2"])
def test_grad_scale_and_pruning(cuda, kname, mode, scale):
    """grad_scale and prune_thr = 0.1 on 9 workgroups: the stored gradient and the pruned count (per-wave atomics
    summed over the grid) equal the oracle's; pruned_count leaves the alignment padding out."""
    sizes = [8191, 5]                      # offsets 0 and 8192: 1 + 11 elements of padding
    n = 8192 + 16
    kind, wd_real, wd_lat = KINDS[kname]
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, kind, wd_lat if mode == "lattice" else wd_real, THR, sizes=sizes)
    real = torch.zeros(n, dtype=torch.bool, device=cuda)
    real[:8191] = True
    real[8192:8197] = True
    total = total_real = 0
    for k in range(3):
        g = torch.where(real, cs.g[k].to(cuda), torch.zeros(n, dtype=D, device=cuda))
        space.grad.copy_(g)
        before = _snap(opt)
        r = _step_and_check(f"prune {mode} {kname} scale={scale:.3f} t={k + 1}", cs, opt, before,
                            lambda: opt.step(grad_scale=scale), 0, n, 0, scale,
                            exact=not (kname.endswith("_l2") and k > 0))
        total += r.pruned
        total_real += int((~((g * oo.f32(scale)).abs() > oo.f32(THR)) & real).sum())
    assert int(opt.pruned) == total and total_real > 0
    assert opt.pruned_count(3) == total_real == total - 3 * 12


# ------------------------------------------------------------------------------------------ skip
@pytest.mark.parametrize("kname", ["adam", "sgd"])
def test_skip_flag(cuda, kname):
    """A nonzero skip flag: every buffer keeps its bits, no tick, done stays 0; the next step is a normal step."""
    cs = oo.case("real", 3 * 1024 + 16)
    space, opt = _opt(cuda, cs, KINDS[kname][0], prune=THR)
    sh = opt.attach_shadow(0, 1024)
    skip = torch.zeros(1, device=cuda)
    for k in range(2):
        space.grad.copy_(cs.g[k])
        before = _snap(opt)
        sh0, pr0 = sh.clone(), int(opt.pruned)
        skip.fill_(float("nan") if k else 1.0)      # (any nonzero value skips: the NaN guard's flag may be NaN)
        opt.step(grad_scale=0.5, skip=skip)
        _unchanged(opt, before)
        assert float(opt.step_t) == k and int(opt.done) == 0 and int(opt.pruned) == pr0 and torch.equal(sh, sh0)
        skip.zero_()
        _step_and_check(f"skip {kname} t={k + 1}", cs, opt, before, lambda: opt.step(grad_scale=0.5, skip=skip),
                        0, cs.n, 0, 0.5)


# ------------------------------------------------------------------------------------------ parts and limit
@pytest.mark.parametrize("mode", MODES)
def test_parts_and_limit(cuda, mode):
    """Three parts stepped in the order 2, 0, 1, each with its own step / done slot; the scratch past limit() keeps
    its sentinel in p, g, m and v although the launches scale, prune and store the gradient."""
    sizes = [2048, 1000, 4096]
    n = 2048 + 1008 + 4096
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, "adam", prune=THR, sizes=sizes, extra=16)
    opt.limit(n)
    opt.partition([2048, 3056])
    for x in _bufs(opt).values():
        x[n:] = S
    for k in range(3):
        space.grad[:n].copy_(cs.g[k])
        for i in (2, 0, 1):
            lo, hi = opt.bounds[i]
            before = _snap(opt)
            _step_and_check(f"parts {mode} part={i} t={k + 1}", cs, opt, before,
                            lambda: opt.step(grad_scale=0.5, part=i), lo, hi, i, 0.5)
            _unchanged(opt, before, 0, lo)
            _unchanged(opt, before, hi, None)
        assert opt.step_t.tolist() == [k + 1.0] * 3
    for x in _bufs(opt).values():
        assert bool((x[n:] == S).all())


# ------------------------------------------------------------------------------------------ hole
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hole_lo", [0, 2048, 8192 - 1024])
def test_hole(cuda, hole_lo, mode):
    """fuse_range: step() leaves the hole's sentinels alone and updates everything else; step_fused steps the hole
    alone, with its own step / done slot, capped to one workgroup or not."""
    n, hn = 8192, 1024
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, "adam")
    slot = opt.fuse_range(hole_lo, hole_lo + hn)
    assert slot == 1
    for k in range(2):
        space.grad.copy_(cs.g[k])
        for x in _bufs(opt).values():
            x[hole_lo:hole_lo + hn] = S
        before = _snap(opt)
        _step_and_check(f"hole lo={hole_lo} {mode} t={k + 1}", cs, opt, before, lambda: opt.step(grad_scale=0.5),
                        0, n, 0, 0.5, hole=(hole_lo, hn))
        _unchanged(opt, before, hole_lo, hole_lo + hn)
        assert float(opt.step_t[slot]) == k and int(opt.done[slot]) == 0
        # the hole itself: the case's data there, one launch over it alone
        for key, src in (("p", cs.p), ("g", cs.g[k]), ("m", cs.m), ("v", cs.v)):
            _bufs(opt)[key][hole_lo:hole_lo + hn].copy_(src[hole_lo:hole_lo + hn])
        before = _snap(opt)
        _step_and_check(f"hole-fused lo={hole_lo} {mode} grid={k} t={k + 1}", cs, opt, before,
                        lambda: opt.step_fused(grad_scale=0.5, max_grid=k), hole_lo, hole_lo + hn, slot, 0.5)
        _unchanged(opt, before, 0, hole_lo)
        _unchanged(opt, before, hole_lo + hn, None)
        assert float(opt.step_t[0]) == k + 1 and int(opt.done[0]) == 0


# ------------------------------------------------------------------------------------------ slab-fed update
def _slab_batch(space, jobs, lo=0):
    b = SlabBatch()
    for j in jobs:
        b.add(j.slab, space.grad[lo + j.off:lo + j.hi], j.groups, j.rows, j.width, j.ld)
    return b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kname,on", [("adam", False), ("adam", True), ("adamw", True), ("adam_l2", True)])
def test_slab_fed_update(cuda, kname, on, mode):
    """The update that sums its gradient slabs itself: adjacent jobs, a merged 16-element gap (left unstepped by the
    kernel as by the oracle), a 64-element gap that is a real parameter (stepped), rows 1 .. 130, widths 4 .. 2048,
    padded rows, several groups; scale and pruning off and on.  The gradient the launch reads in a job's range is
    the slab's alone: the buffer holds a sentinel there."""
    n, hole, specs = oo.SLAB_LAYOUTS["mixed"]
    kind, wd_real, wd_lat = KINDS[kname]
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, kind, wd_lat if mode == "lattice" else wd_real, THR if on else 0.0)
    scale = 0.5 if on else 1.0
    jobs = oo.layout_jobs(cs, specs, cuda)
    total = 0
    for k in range(3):
        space.grad.copy_(cs.g[k])
        for j in jobs:
            space.grad[j.off:j.hi] = S
        before = _snap(opt)
        batch = _slab_batch(space, jobs)
        r = _step_and_check(f"slabs {mode} {kname} on={int(on)} t={k + 1}", cs, opt, before,
                            lambda: opt.step(grad_scale=scale, slabs=batch), 0, n, 0, scale, jobs=jobs,
                            exact=not (kname.endswith("_l2") and k > 0))
        assert not bool(r.stepped[248:264].any()) and bool(r.stepped[328:392].all())
        total += r.pruned
    assert int(opt.pruned) == total


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_slab_fed_update_around_the_hole(cuda, scale, mode):
    """A 48-element gap between two jobs that holds the 16-element hole: not merged, so its other 32 elements are
    stepped by the regular pass and the hole keeps its sentinels."""
    n, hole, specs = oo.SLAB_LAYOUTS["hole"]
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, "adam")
    opt.fuse_range(hole[0], hole[0] + hole[1])
    jobs = oo.layout_jobs(cs, specs, cuda)
    for k in range(2):
        space.grad.copy_(cs.g[k])
        for x in _bufs(opt).values():
            x[hole[0]:hole[0] + hole[1]] = S
        before = _snap(opt)
        batch = _slab_batch(space, jobs)
        r = _step_and_check(f"slabs-hole {mode} scale={scale} t={k + 1}", cs, opt, before,
                            lambda: opt.step(grad_scale=scale, slabs=batch), 0, n, 0, scale, jobs=jobs, hole=hole)
        assert bool(r.stepped[192:208].all()) and bool(r.stepped[224:240].all())
        _unchanged(opt, before, hole[0], hole[0] + hole[1])


@pytest.mark.parametrize("name", sorted(oo.SLAB_REFUSALS))
def test_slab_refusals(cuda, name):
    """Five disjoint skip intervals, overlapping jobs, a job inside the hole, width 2: the launcher returns an error
    and no buffer changes."""
    n, hole, specs = oo.SLAB_REFUSALS[name]
    cs = oo.case("real", n)
    space, opt = _opt(cuda, cs, "adam")
    if hole[1]:
        opt.fuse_range(hole[0], hole[0] + hole[1])
    space.grad.copy_(cs.g[0])
    jobs = oo.layout_jobs(cs, specs, cuda)
    before = _snap(opt)
    batch = _slab_batch(space, jobs)
    with pytest.raises(RuntimeError, match="HIP status 1"):
        opt.step(slabs=batch)
    _unchanged(opt, before)
    assert float(opt.step_t[0]) == 0 and int(opt.done[0]) == 0


def test_e4m3_shadow_refuses_a_grid_beyond_the_amax_partials(cuda):
    """Every workgroup writes one |w|-max partial: an e4m3 shadow with slab jobs whose extra workgroups push the grid
    past the 4096 partials is refused before anything is launched."""
    n = 4 * 4096 + 1024
    cs = oo.case("real", n)
    space, opt = _opt(cuda, cs, "adam")
    fp8 = Fp8Scales(2, cuda)
    opt.attach_shadow(4 * 4096, n, fp8, 1)
    space.grad.copy_(cs.g[0])
    slab = torch.ones(4096, 4, device=cuda)
    before = _snap(opt)
    sh, sh8, amax = opt.shadow.clone(), opt.shadow8.view(torch.uint8).clone(), fp8.amax.clone()
    batch = SlabBatch()
    batch.add(slab, space.grad[:4 * 4096], 4096, 1, 4)       # 4096 one-quad workgroups + the regular ones
    with pytest.raises(RuntimeError, match="HIP status 1"):
        opt.step(slabs=batch)
    _unchanged(opt, before)
    assert torch.equal(opt.shadow, sh) and torch.equal(opt.shadow8.view(torch.uint8), sh8)
    assert torch.equal(fp8.amax, amax) and float(opt.step_t) == 0 and int(opt.done) == 0


# ------------------------------------------------------------------------------------------ shadows
@pytest.mark.parametrize("mode", MODES)
def test_bf16_shadow_clipped_to_a_part(cuda, mode):
    """A shadow over [1024, 3072) of a space cut at 2048 and 4096: a part's launch writes the shadow of its own
    elements (the cast of the kernel's p, exactly) and leaves the rest of it alone."""
    n = 6144
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, "adam")
    opt.partition([2048, 4096])
    sh = opt.attach_shadow(1024, 3072)
    space.grad.copy_(cs.g[0])
    init = sh.clone()
    oo.assert_equal("initial shadow", init, oo.shadows(space.flat, (1024, 3072))[0])
    for i, (a, b) in ((1, (1024, 2048)), (2, (0, 0)), (0, (0, 1024))):
        lo, hi = opt.bounds[i]
        before, sh0 = _snap(opt), sh.clone()
        _step_and_check(f"shadow {mode} part={i}", cs, opt, before, lambda: opt.step(part=i), lo, hi, i)
        new = oo.shadows(space.flat, (1024, 3072))[0]
        oo.assert_equal(f"shadow of part {i}", sh[a:b], new[a:b])
        keep = torch.ones(2048, dtype=torch.bool, device=cuda)
        keep[a:b] = False
        assert torch.equal(sh[keep], sh0[keep])
    oo.assert_equal("shadow", sh, oo.shadows(space.flat, (1024, 3072))[0])
    assert not torch.equal(sh, init)


@pytest.mark.parametrize("mode", MODES)
def test_e4m3_shadow_and_amax(cuda, mode):
    """The e4m3 shadow: bytes == the oracle's cast of the kernel's p times qs (at most 0.1 % of the bytes may differ,
    the hardware converter's cap of tests/test_conv_gpu.py), the amax partials max to max |p| exactly, and update()
    turns them into scale = amax 2^margin / 448, qs = 1 / scale (2 ulp) and re-arms them."""
    n, slot, margin = 8192, 1, 1.0
    cs = oo.case(mode, n)
    space, opt = _opt(cuda, cs, "adam")
    fp8 = Fp8Scales(3, cuda, margin=margin)
    opt.attach_shadow(0, n, fp8, slot)
    for k in range(2):
        space.grad.copy_(cs.g[k])
        qs = float(fp8.qs[slot])
        before = _snap(opt)
        _step_and_check(f"e4m3 {mode} t={k + 1}", cs, opt, before, lambda: opt.step(), 0, n, 0)
        sh, b8, wmax = oo.shadows(space.flat, (0, n), qs)
        oo.assert_equal("bf16 shadow", opt.shadow, sh)
        diff = float((opt.shadow8.view(torch.uint8) != b8).double().mean())
        print(f"ORACLE e4m3 {mode} t={k + 1} differing bytes {diff:.5f}")
        assert diff <= 1e-3
        assert float(fp8.amax[slot].max()) == wmax > 0 and float(fp8.amax[0].max()) == 0 == float(fp8.amax[2].max())
        others = fp8.scale.clone(), fp8.qs.clone()
        fp8.update()
        torch.cuda.synchronize()
        ref_s = wmax * 2.0 ** margin / FP8_E4M3_MAX
        ulp2 = 2 * 2.0 ** -23
        assert abs(float(fp8.scale[slot]) - ref_s) <= ulp2 * ref_s
        assert abs(float(fp8.qs[slot]) - 1.0 / float(fp8.scale[slot])) <= ulp2 / float(fp8.scale[slot])
        assert float(fp8.amax.abs().max()) == 0
        for i in (0, 2):     # (tensors nobody produced keep their scale)
            assert torch.equal(fp8.scale[i], others[0][i]) and torch.equal(fp8.qs[i], others[1][i])


def test_fp8_scale_update(cuda):
    """Fp8Scales.update() alone: 7 tensors with partials in random slots (slot 4095 among them); the tensor with
    all-zero partials keeps the bits of its scale and qs, the others follow the formula, every partial is re-armed."""
    gen = torch.Generator().manual_seed(3)
    nt, margin = 7, 2.0
    fp8 = Fp8Scales(nt, cuda, margin=margin)
    prev_s = (0.5 + torch.rand(nt, generator=gen)).to(cuda)
    prev_q = (0.5 + torch.rand(nt, generator=gen)).to(cuda)     # (not 1 / scale: bits that only a copy reproduces)
    fp8.scale.copy_(prev_s)
    fp8.qs.copy_(prev_q)
    parts = torch.zeros(nt, Fp8Scales.PARTS)
    for i in range(nt):
        if i == 3:
            continue
        idx = torch.randperm(Fp8Scales.PARTS, generator=gen)[:5 + i]
        parts[i, idx] = torch.rand(5 + i, generator=gen) * 10 ** (i - 3)
    parts[5, 4095] = 77.0
    parts[6, 0] = 1e-3
    fp8.amax.copy_(parts)
    fp8.update()
    torch.cuda.synchronize()
    assert float(fp8.amax.abs().max()) == 0
    ulp2 = 2 * 2.0 ** -23
    for i in range(nt):
        if i == 3:
            assert torch.equal(fp8.scale[i], prev_s[i]) and torch.equal(fp8.qs[i], prev_q[i])
            continue
        ref = float(parts[i].max().double()) * 2.0 ** margin / FP8_E4M3_MAX
        s = float(fp8.scale[i])
        assert abs(s - ref) <= ulp2 * ref and abs(float(fp8.qs[i]) - 1.0 / s) <= ulp2 / s, i


# ------------------------------------------------------------------------------------------ fused FC Adam
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("M,N,K,cfg", [(192, 256, 512, 0), (192, 256, 512, 1), (256, 256, 512, 0), (256, 256, 512, 1),
                                       (256, 256, 512, 2)])
def test_fused_fc_adam(cuda, M, N, K, cfg, scale):
    """gemm_wgrad_adam on a range in the middle of a larger space: p, m, v within the bounds for the gradient
    dW = gemm_wgrad(dY, A) (the same accumulators; dW itself is held to fp64 in tests/test_gemm_gpu.py), the bf16
    shadow the exact cast of the kernel's p, the neighbours' sentinels intact, one tick per step and none when
    skipped.  (cfg 2 runs the M reduction in pairs of 64: M % 128 == 0 only.)"""
    lo, nk = 1024, N * K
    n = lo + nk + 1024
    cs = oo.case("real", n)
    space, opt = _opt(cuda, cs, "adam", lr=1e-3, sizes=[lo, nk, 1024])
    slot = opt.fuse_range(lo, lo + nk)
    sh = opt.attach_shadow(lo, lo + nk)
    for x in (space.flat, opt.m, opt.v, space.grad):
        x[:lo] = S
        x[lo + nk:] = S
    skip = torch.zeros(1, device=cuda)
    gen = torch.Generator().manual_seed(100 * M + cfg)
    hp = _hyper(cs, opt, scale)
    for k in range(3):
        dY = (torch.randn(M, N, generator=gen) * 1e-2).bfloat16().to(cuda)
        A = torch.randn(M, K, generator=gen).bfloat16().to(cuda)
        dW = gemm_wgrad(dY, A, cfg=cfg).reshape(-1)
        before = _snap(opt)
        gemm_wgrad_adam(dY, A, opt, lo, slot, skip=skip, grad_scale=scale, cfg=cfg)
        torch.cuda.synchronize()
        r = oo.step(hp, before["p"][lo:lo + nk], dW, before["m"][lo:lo + nk], before["v"][lo:lo + nk], float(k),
                    float(opt.lr_t))
        got = dict(p=space.flat[lo:lo + nk], m=opt.m[lo:lo + nk], v=opt.v[lo:lo + nk])
        r.g = None                                   # (dW is never stored)
        _compare(f"fc M={M} cfg={cfg} scale={scale} t={k + 1}", "real", r, got)
        oo.assert_equal("bf16 shadow", sh, oo.shadows(space.flat, (lo, lo + nk))[0])
        _unchanged(opt, before, 0, lo)
        _unchanged(opt, before, lo + nk, None)
        assert float(opt.step_t[slot]) == k + 1 and int(opt.done[slot]) == 0 and float(opt.step_t[0]) == 0
    skip.fill_(1.0)
    before, sh0 = _snap(opt), sh.clone()
    gemm_wgrad_adam(dY, A, opt, lo, slot, skip=skip, grad_scale=scale, cfg=cfg)
    _unchanged(opt, before)
    assert torch.equal(sh, sh0) and float(opt.step_t[slot]) == 3 and int(opt.done[slot]) == 0


# ------------------------------------------------------------------------------------------ graph replay
def test_graph_replay(cuda):
    """The plain update captured once and replayed 3 times, the learning rate changed by set_lr between replays:
    3 oracle steps with those rates, and the last-workgroup tick survives replay."""
    n = 3 * 1024 + 16
    cs = oo.case("real", n)
    warm = _opt(cuda, cs, "adam")[1]
    warm.step()                                      # (the launch path's one-time work, outside the capture)
    space, opt = _opt(cuda, cs, "adam")
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    assert float(opt.step_t) == 0                    # (capture runs nothing)
    for k, lr in enumerate((1e-2, 3e-3, 1e-3)):
        opt.set_lr(lr)
        space.grad.copy_(cs.g[k])
        before = _snap(opt)
        _step_and_check(f"graph t={k + 1}", cs, opt, before, gph.replay, 0, n, 0, 0.5)
        assert float(opt.lr_t) == oo.f32(lr)
