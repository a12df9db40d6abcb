"""The optimizer oracle (tests/optim_oracle.py) checked against torch.optim, against the project's CPU path and
against itself, no GPU: it is the reference tests/test_optim_exact_gpu.py holds the HIP kernels to."""
import pytest
import torch

import optim_oracle as oo
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.optim import (FlatParamSpace, FusedOptimizer,
                                                                                       FP8_E4M3_MAX)

D = torch.float64


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 0.01), ("adamw", 0.01), ("sgd", 0.0), ("sgd", 0.01)])
def test_oracle_ideal_mode_is_torch_optim(kind, wd):
    """Ideal mode (float64 hyper-parameters as given) == torch.optim on float64 parameters, 20 steps, rtol 1e-12."""
    gen = torch.Generator().manual_seed(11)
    n, lr = 257, 1e-2
    ref_p = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=D))
    ref = {"adam": lambda: torch.optim.Adam([ref_p], lr=lr, weight_decay=wd),
           "adamw": lambda: torch.optim.AdamW([ref_p], lr=lr, weight_decay=wd),
           "sgd": lambda: torch.optim.SGD([ref_p], lr=lr, momentum=0.9, weight_decay=wd)}[kind]()
    hp = oo.Hyper(kind, wd=wd, ideal=True)
    p, m = ref_p.detach().clone(), torch.zeros(n, dtype=D)
    v = None if kind == "sgd" else torch.zeros(n, dtype=D)
    for t in range(20):
        g = torch.randn(n, generator=gen, dtype=D)
        ref_p.grad = g.clone()
        ref.step()
        r = oo.step(hp, p, g, m, v, float(t), lr)
        p, m, v = r.p, r.m, r.v
        assert r.t == t + 1 and torch.equal(r.g, g)          # (no scale, no pruning: the gradient is left alone)
        assert torch.allclose(p, ref_p.detach(), rtol=1e-12, atol=0), (t, float((p - ref_p.detach()).abs().max()))


def _host_space(extra=8):
    gen = torch.Generator().manual_seed(5)
    shapes = [(33, 7), (5,), (64, 3, 3, 3), (100,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    return FlatParamSpace([(f"p{i}", q) for i, q in enumerate(params)], "cpu", extra=extra), gen


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 0.01), ("adamw", 0.01), ("sgd", 0.0), ("sgd", 0.01)])
def test_oracle_matches_host_path(kind, wd):
    """FusedOptimizer on a CPU space (_step_host) against the oracle: grad_scale 0.5, prune_thr 0.1, two parts and a
    limit.  The host path is another fp32 evaluation of the same operation (torch's elementwise kernels, a divide by
    sqrt(bc2) where the kernel multiplies by its reciprocal): it is held to 4x the bounds derived for the kernel."""
    space, gen = _host_space()
    opt = FusedOptimizer(space, kind, lr=1e-2, weight_decay=wd, prune_thr=oo.PRUNE_THR)
    end = space.extra_off
    opt.limit(end)
    cut = space.offsets[2]
    opt.partition([cut])
    assert opt.bounds == [(0, cut), (cut, end)]
    hp = oo.Hyper(kind, wd=wd, grad_scale=0.5, prune_thr=oo.PRUNE_THR)
    real = torch.zeros(space.numel, dtype=torch.bool)
    for q, o in zip(space.params, space.offsets):
        real[o:o + q.numel()] = True
    st = "buf" if kind == "sgd" else "m"
    total = total_real = 0
    for t in range(3):
        space.grad[:end] = torch.where(real[:end], 0.3 * torch.randn(end, generator=gen), torch.zeros(end))
        space.grad[end:] = space.flat[end:] = oo.SENTINEL      # the scratch past the limit
        lr = float(opt.lr_t.item())
        before = [x.clone() for x in (space.flat, space.grad, getattr(opt, st))]
        before.append(None if kind == "sgd" else opt.v.clone())
        opt.step(grad_scale=0.5)
        for lo, hi in opt.bounds:
            r = oo.step(hp, before[0][lo:hi], before[1][lo:hi], before[2][lo:hi],
                        None if kind == "sgd" else before[3][lo:hi], float(t), lr)
            assert r.ambiguous == 0
            total += r.pruned
            total_real += int((~((0.5 * before[1][lo:hi].to(D)).abs() > oo.f32(oo.PRUNE_THR)) & real[lo:hi]).sum())
            got = dict(p=space.flat[lo:hi], m=getattr(opt, st)[lo:hi], g=space.grad[lo:hi])
            ref = dict(p=(r.p, r.bp), m=(r.m, r.bm), g=(r.g, r.bg))
            if kind != "sgd":
                got["v"], ref["v"] = opt.v[lo:hi], (r.v, r.bv)
            for k, x in got.items():
                ratio = oo.worst_ratio((x.to(D) - ref[k][0]).abs(), 4 * ref[k][1])
                assert ratio <= 1.0, (kind, t, k, ratio)
        assert torch.equal(opt.step_t, torch.full((2,), t + 1.0))
        assert bool((space.flat[end:] == oo.SENTINEL).all()) and bool((space.grad[end:] == oo.SENTINEL).all())
    assert int(opt.pruned.item()) == total
    # pruned_count leaves the alignment padding out: its zero gradients are pruned at every step
    pad = end - space.n_real
    assert opt.pruned_count(3) == total - 3 * pad
    assert opt.pruned_count(3) == total_real > 0


def _chain(cs, hp, n_steps=None, lr=1e-2):
    """The oracle's own trajectory over the case's gradients: the Results of each step."""
    p, m, v = cs.p, cs.m, (None if hp.kind == "sgd" else cs.v)
    out = []
    for t in range(n_steps or cs.steps):
        r = oo.step(hp, p, cs.g[t], m, v, float(t), oo.f32(lr))
        out.append(r)
        p, m, v = r.p.to(torch.float32), r.m, r.v
    return out


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adamw", 0.01), ("sgd", 0.0)])
def test_lattice_is_exact(kind, wd, scale):
    """The lattice's conditions: every m, v, scaled and written-back gradient of 3 steps is an fp32 value, and no
    prune decision is near the threshold."""
    for n in (16, 3 * 1024 + 16, 8192):
        cs = oo.case("lattice", n)
        for x in (cs.p, cs.m, cs.v, *cs.g):
            assert oo.is_f32(x) and float(x.abs().max()) <= 64
        hp = oo.Hyper(kind, betas=cs.betas, wd=wd, grad_scale=scale, prune_thr=oo.PRUNE_THR, momentum=0.5)
        for t, r in enumerate(_chain(cs, hp)):
            assert r.exact and r.ambiguous == 0, (n, t)
            assert n < 1024 or r.pruned > n // 16      # (one gradient in eight is zero)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_lattice_with_l2_decay_is_exact_for_one_step(kind):
    """wd = 0.25 on lattice weights: g + wd p is on the lattice for the first step; p then leaves it."""
    cs = oo.case("lattice", 3 * 1024 + 16)
    hp = oo.Hyper(kind, betas=cs.betas, wd=0.25, grad_scale=0.5, prune_thr=oo.PRUNE_THR, momentum=0.5)
    assert _chain(cs, hp, 1)[0].exact


def test_real_seeds_have_no_ambiguous_prune_decision():
    """No |g * scale| of the REAL cases the GPU tests use lies within 4u thr of the threshold, for any scale."""
    sizes = sorted({n for n, _ in oo.SIZES} | {1040, 1027, 8192})
    for n in sizes:
        cs = oo.case("real", n)
        for scale in oo.SCALES:
            hp = oo.Hyper("adam", grad_scale=scale, prune_thr=oo.PRUNE_THR)
            for t in range(cs.steps):
                r = oo.step(hp, cs.p, cs.g[t], cs.m, cs.v, float(t), 1e-3)
                assert r.ambiguous == 0, (n, scale, t)
                assert n < 1024 or 0 < r.pruned < n
    for name, (n, hole, specs) in oo.SLAB_LAYOUTS.items():
        cs = oo.case("real", n)
        hp = oo.Hyper("adam", grad_scale=0.5, prune_thr=oo.PRUNE_THR)
        r = oo.step(hp, cs.p, cs.g[0], cs.m, cs.v, 0.0, 1e-3, hole=hole, jobs=oo.layout_jobs(cs, specs))
        assert r.ambiguous == 0, name


def test_e4m3_oracle_is_torch_cast():
    """The e4m3 oracle (float64 product -> fp32 -> clamp -> torch's cast) differs from the cast of the fp32 product
    on 0 % of the inputs the GPU test quantises, values beyond +-448 included."""
    cs = oo.case("real", 8192)
    p = cs.p.clone()
    p[:4] = torch.tensor([1e4, -1e4, 0.0, -0.0], dtype=D)
    amax = float(p[8:].abs().max())
    for margin in (0.0, 1.0):
        qs = oo.f32(1.0 / oo.f32(amax * 2.0 ** margin / FP8_E4M3_MAX))
        ours = oo.e4m3_bytes(p * qs)
        theirs = (p.float() * torch.tensor(qs, dtype=torch.float32)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX) \
            .to(torch.float8_e4m3fn).view(torch.uint8)
        assert int((ours != theirs).sum()) == 0
    sh, _, wmax = oo.shadows(p.float(), (8, 8192))
    assert torch.equal(sh, p[8:].float().bfloat16().to(D)) and wmax == amax


@pytest.mark.parametrize("name", sorted(oo.SLAB_LAYOUTS))
def test_slab_model_against_plain_sums(name):
    """The jobs' gradients == slab.sum(1) scattered by hand; merged gaps are left unstepped, a 64-element gap and a
    gap holding the hole are stepped outside the hole."""
    n, hole, specs = oo.SLAB_LAYOUTS[name]
    cs = oo.case("lattice", n)
    jobs = oo.layout_jobs(cs, specs)
    gsum, in_job, skipped, _ = oo.slab_model(jobs, n, hole)
    ref = torch.zeros(n, dtype=D)
    own = torch.zeros(n, dtype=torch.bool)
    for j in jobs:
        for gi in range(j.groups):
            rows = j.slab[gi * j.rows:(gi + 1) * j.rows, :j.width].to(D)
            ref[j.off + gi * j.width:j.off + (gi + 1) * j.width] = rows.sum(0)
            own[j.off + gi * j.width:j.off + (gi + 1) * j.width] = True
    assert torch.equal(gsum, ref) and torch.equal(in_job, own)
    hp = oo.Hyper("adam", betas=cs.betas)
    r = oo.step(hp, cs.p, cs.g[0], cs.m, cs.v, 0.0, 1e-2, hole=hole, jobs=jobs)
    unstepped = ~r.stepped
    if name == "mixed":
        assert oo.skip_intervals(jobs, n, hole) == [(64, 328), (392, 6668), (7168, 7172)]
        assert unstepped.nonzero().flatten().tolist() == list(range(248, 264))       # the merged 16-element gap
        assert bool(r.stepped[328:392].all())                                        # the 64-element gap
    else:
        assert oo.skip_intervals(jobs, n, hole) == [(128, 192), (240, 420), (2048, 2116)]
        assert unstepped.nonzero().flatten().tolist() == list(range(208, 224))       # the hole alone
    for x, y in ((r.p, cs.p), (r.m, cs.m), (r.v, cs.v), (r.g, cs.g[0])):
        assert torch.equal(x[unstepped], y[unstepped])
    # slab elements always get their gradient stored; the others keep theirs (no scale, no pruning)
    assert torch.equal(r.g[own], ref[own]) and torch.equal(r.g[~own], cs.g[0][~own])
    assert bool((r.m[r.stepped] != cs.m[r.stepped]).any())


@pytest.mark.parametrize("name", sorted(oo.SLAB_REFUSALS))
def test_slab_model_refusals(name):
    n, hole, specs = oo.SLAB_REFUSALS[name]
    with pytest.raises(ValueError):
        oo.skip_intervals(oo.layout_jobs(oo.case("lattice", n), specs), n, hole)


def test_skip_changes_nothing():
    cs = oo.case("real", 1040)
    r = oo.step(oo.Hyper("adam", grad_scale=0.5, prune_thr=0.1), cs.p, cs.g[0], cs.m, cs.v, 4.0, 1e-3, skip=True)
    assert r.t == 4.0 and r.pruned == 0 and not bool(r.stepped.any())
    assert all(torch.equal(a, b) for a, b in ((r.p, cs.p), (r.g, cs.g[0]), (r.m, cs.m), (r.v, cs.v)))
