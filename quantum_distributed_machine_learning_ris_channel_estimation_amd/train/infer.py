"""Test-time hierarchical estimation on the HIP kernels (the model side of ``Test.py``'s sweep).

Reference (Test.py:140-214): per test batch, classify the scenario with the classical SC and the quantum
SC, bucket the samples by predicted scenario in a Python loop, run each bucket through its expert
``Conv_s`` and the shared ``CE`` (all under DataParallel, on cuDNN / cuBLAS).

Here, per chunk of ``chunk`` samples (one static buffer set; graph-friendly, no host sync inside):
  gather      the chunk's pilots into the experts-in-channels conv input (csrc/hip/gather.hip with a
              zero stream stride: every expert's channel pair carries the same sample)
  classify    SC_P128: csrc/hip/sc.hip forward (argmax written in-kernel); QSC_P128: preprocess +
              circuit (clean master weights) + a thread-per-sample head (csrc/hip/qsc*.hip, qsim*.hip)
  experts     the conv / BN (running statistics) / ReLU stack of ALL experts on every sample
              (csrc/hip/conv.hip, one launch per layer): at these sizes evaluating the three small
              experts densely costs less than sorting samples into buckets
  routed FC   csrc/hip/gemm.hip forward GEMM whose A-operand loads read row ``i * E + expert[i]`` of the
              expert features: the top-1 routing is fused into the GEMM (no permutation, no scatter)
  mixed FC    (soft routing) the same GEMM over ALL expert rows, the classifier's posterior combining each
              sample's three product rows in its epilogue (``estimate_mixed``, csrc/hip/gemm.hip EPI_MIX)

``dtype="fp8"``: the shared FC in OCP e4m3, the precision the fp8 estimator is trained in (``engine``'s definition:
``quantise_rows_e4m3`` and the fp8 estimates).  The last expert launch becomes the row-quantising BN + ReLU apply
(csrc/hip/conv.hip qd_bn_relu_rows_f8: every FC-operand row (sample, expert) gets its own power-of-two scale, the bf16
operand is never written), the weights are quantised per output channel once (and by ``refresh``), and the routed /
mixed FC are qd_gemm_fwd_rows_f8 / qd_gemm_fwd_mix_rows_f8, which dequantise by row and column in their epilogues.
Nothing is calibrated, so a sample's estimate does not depend on its chunk or its neighbours, and test-time BN
adaptation needs no extra step.

``HIPInference.session(batch, ...)`` (``InferSession``): the low-latency path for ONE request of 1..16 samples -- a
pilot frame of the system's 9 user streams, not a sweep chunk.  Input packing, classifier, routing, the experts and
the FC are one captured graph on one stream; the FC is the skinny forward (csrc/hip/gemm_skinny.hip), which streams
the weight once over the whole chip instead of tiling 144 rows.
"""
from __future__ import annotations

import copy
import ctypes
from typing import Optional, Sequence

import torch
import torch.nn as nn

from .. import _native as nat
from ..models.estimators import QSC_P128, SC_P128, pilot_grid
from ..ops.optim import FlatParamSpace

_p, _i, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


class HIPInference:
    def __init__(self, convs: Sequence[nn.Module], fc: nn.Module, pilot_num: int, device, chunk: int = 2304,
                 sc: Optional[SC_P128] = None, qsc: Optional[QSC_P128] = None, dtype: str = "bf16"):
        from ..ops.conv import ConvStackHIP
        from ..ops.qsc import QSCStepHIP
        from ..ops.sc import SCStepHIP
        from .engine import HDCEModel, _infer_dtype
        self.dev = torch.device(device)
        self.chunk = chunk
        self.dtype = _infer_dtype(dtype)
        if self.dtype == "fp8" and chunk % 144:
            raise ValueError(f"HIPInference(dtype='fp8'): chunk {chunk} is not a multiple of 144 (whole GEMM tiles)")
        self.H, self.W = pilot_grid(pilot_num)
        self.E = len(convs)
        self.pilot_num = pilot_num
        # the estimator: an HDCEModel holding the checkpoint's experts + FC (its grouped buffers are what
        # the conv kernels read), eval mode
        m = HDCEModel(pilot_num, self.dev, "bf16", self.E)
        with torch.no_grad():
            for e in range(self.E):
                m.convs[e].load_state_dict(convs[e].state_dict())
            m.fc.load_state_dict(fc.state_dict())
        self.model = m
        self.conv = ConvStackHIP(m, 1, chunk)
        self.W_lp = m.fc_w.detach().to(torch.bfloat16).contiguous()
        self.b_lp = m.fc_b.detach().to(torch.bfloat16).contiguous()
        self.W8 = self.cs = None
        if self.dtype == "fp8":
            self.conv.rows_f8 = True    # (eval forwards return the e4m3 rows; their scales in conv.rs)
            self._quantise_fc()
            # FwdM8P (MX MFMA, producer waves) where K allows, else the non-scaled e4m3 MFMA
            self.f8_cfg = 2 if self.W8.shape[1] % 256 == 0 else 0
        # classifiers: private copies whose parameters live in flat spaces (the kernels' layout)
        self.sc = self.qsc = None
        if sc is not None:
            self._sc_mod = copy.deepcopy(sc).to(self.dev).eval()
            self.sc = SCStepHIP(self._sc_mod, FlatParamSpace(list(self._sc_mod.named_parameters()), self.dev))
        if qsc is not None:
            self._qsc_mod = copy.deepcopy(qsc).to(self.dev).eval()
            self.qsc = QSCStepHIP(self._qsc_mod, FlatParamSpace(list(self._qsc_mod.named_parameters()), self.dev),
                                  chunk, n_groups=1)
        plane = 2 * self.H * self.W
        self.xq = torch.zeros(chunk, 2, self.H, self.W, device=self.dev)
        self.x1 = torch.zeros(chunk, 2 * self.E, self.H, self.W, device=self.dev)
        self.idx = torch.zeros(chunk, dtype=torch.int64, device=self.dev)
        self.pred = torch.zeros(chunk, dtype=torch.int64, device=self.dev)
        self.Y = torch.empty(chunk, self.W_lp.shape[0], device=self.dev, dtype=torch.bfloat16)
        self.wmix = torch.zeros(chunk, self.E, device=self.dev)    # (estimate_mixed's weights of the chunk)
        self._logp = {}                                             # (classify(return_logp=True): per classifier)
        self._gather = nat.fn(nat.hip_lib(), "qd_gather_step", [_p, _p, _l, _p, _p, _p, _l, _i, _i, _i, _i, _p])
        self._plane = plane

    def _quantise_fc(self) -> None:
        """The e4m3 FC weight with one power-of-two scale per output channel, from the fp32 master."""
        from .engine import quantise_rows_e4m3
        W8, cs = quantise_rows_e4m3(self.model.fc_w.detach())
        if self.W8 is None:
            self.W8, self.cs = W8.contiguous(), cs.contiguous()
        else:
            self.W8.copy_(W8)
            self.cs.copy_(cs)

    def session(self, batch: int, which: Optional[str] = "quantum", routing: str = "hard", shots: int = 0,
                seed: int = 0, noise=None, trajectories: int = 1) -> "InferSession":
        """A low-latency estimate path for requests of exactly ``batch`` (1..16) samples: see ``InferSession``."""
        return InferSession(self, batch, which, routing, shots, seed, noise, trajectories)

    @torch.no_grad()
    def refresh(self, convs: Sequence[nn.Module], fc: nn.Module) -> None:
        """Reload the estimator weights and BN statistics (e.g. once per epoch of a training run: the
        engine's buffers and static launch shapes are kept, the conv weights are re-packed by every forward)."""
        for e in range(self.E):
            self.model.convs[e].load_state_dict(convs[e].state_dict())
        self.model.fc.load_state_dict(fc.state_dict())
        self.W_lp.copy_(self.model.fc_w.detach())
        self.b_lp.copy_(self.model.fc_b.detach())
        if self.dtype == "fp8":
            self._quantise_fc()

    @torch.no_grad()
    def load_bn_stats(self, convs: Sequence[nn.Module]) -> None:
        """Refresh the experts' BN running statistics (views into the grouped buffers the conv kernels
        read) from ``convs``, e.g. after a test-time BN re-estimation."""
        for e in range(self.E):
            src = [m for m in convs[e].modules() if isinstance(m, nn.BatchNorm2d)]
            dst = [m for m in self.model.convs[e].modules() if isinstance(m, nn.BatchNorm2d)]
            for d, s_ in zip(dst, src):
                d.running_mean.copy_(s_.running_mean)
                d.running_var.copy_(s_.running_var)

    @torch.no_grad()
    def recalibrate_bn(self, convs: Sequence[nn.Module], x: torch.Tensor, expert: torch.Tensor,
                       chunk: int = 4096) -> list:
        """Test-time BN re-estimation (``evaluate.recalibrate_bn``, the sweep's bn_adapt option) on the HIP
        training conv forward instead of MIOpen: every expert's BN running statistics become the cumulative
        average of its per-chunk batch statistics over the samples routed to it (torch's momentum=None rule,
        reproduced exactly as momentum 1/k for the k-th chunk of the kernels' running-stat update; chunks
        of fewer than 2 samples are skipped, as there).  Runs on a scratch copy of the experts (the other
        experts' channels of a launch get the same samples and are discarded), writes the new statistics
        into ``convs`` and returns their previous ones for ``evaluate.restore_bn``."""
        from ..ops.conv import ConvStackHIP
        from .engine import HDCEModel
        if getattr(self, "_rc_model", None) is None:
            self._rc_model = HDCEModel(self.pilot_num, self.dev, "bf16", self.E)
        m = self._rc_model
        stacks = {}
        x = x.to(self.dev).contiguous().float()
        expert = expert.to(self.dev)
        saved = []
        for e, conv in enumerate(convs):
            bns = [b for b in conv.modules() if isinstance(b, nn.BatchNorm2d)]
            saved.append([(b.momentum, b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone())
                          for b in bns])
            xe = x[expert == e]
            n = xe.shape[0]
            if n < 2:
                continue
            m.convs[e].load_state_dict(conv.state_dict())
            dst = [b for b in m.convs[e].modules() if isinstance(b, nn.BatchNorm2d)]
            for d in dst:
                d.running_mean.zero_()
                d.running_var.fill_(1.0)
            k = 0
            for lo in range(0, n, chunk):
                c = min(chunk, n - lo)
                if c < 2:
                    continue
                k += 1
                if c not in stacks:
                    stacks[c] = (ConvStackHIP(m, 1, c),
                                 torch.empty(c, 2 * self.E, self.H, self.W, device=self.dev))
                stk, x1 = stacks[c]
                x1.view(c, self.E, 2, self.H, self.W).copy_(xe[lo:lo + c].view(c, 1, 2, self.H, self.W)
                                                            .expand(c, self.E, 2, self.H, self.W))
                m.momentum = 1.0 / k
                stk.forward(x1, training=True)
            m.momentum = 0.1
            for b, d in zip(bns, dst):
                b.running_mean.copy_(d.running_mean)
                b.running_var.copy_(d.running_var)
                b.num_batches_tracked.fill_(k)
        return saved

    def _load(self, x: torch.Tensor, lo: int, n: int) -> None:
        """Samples x[lo:lo+n] -> the classifier input (xq) and the experts-in-channels conv input (x1); the
        chunk's tail (n < chunk) repeats sample lo (its outputs are dropped)."""
        torch.arange(lo, lo + self.chunk, out=self.idx)
        self.idx.clamp_(max=lo + n - 1)
        st = nat.stream_ptr(self.dev)
        nat.check(self._gather(nat.ptr(self.idx), nat.ptr(x), 0, nat.ptr(self.x1), None, None, 0, self.E, 1,
                               self.chunk, self._plane, st), "gather(x1)")
        nat.check(self._gather(nat.ptr(self.idx), nat.ptr(x), 0, None, nat.ptr(self.xq), None, 0, 1, 1,
                               self.chunk, self._plane, st), "gather(xq)")

    @torch.no_grad()
    def classify(self, x: torch.Tensor, which: str, shots: int = 0, seed: int = 0, noise=None,
                 trajectories: int = 1, return_logp: bool = False, exact_noise: bool = False):
        """Predicted scenario (N,) int64 of every sample with the classical ("classical") or quantum SC.
        ``return_logp``: ``(pred, logp)`` with the log-posterior (N, n_classes) fp32 of the same launches -- under
        ``shots`` / ``noise`` the one of the measured <Z_i>, exactly what ``pred`` was taken from.
        ``shots`` > 0 ("quantum" only): the circuit is measured with that many shots per sample; the shot
        stream is keyed by ``seed`` and the chunk index (the counter), the sample's row within its chunk.
        ``noise`` / ``trajectories`` (with ``shots``): measured under that ``ops.quantum.NoiseModel``.
        ``exact_noise`` ("quantum" only; with ``noise`` and no ``shots``): the exact expectation of that noisy
        device instead of a sample of it (``ops.quantum.qsim_mixed``; n <= 8), deterministic."""
        if shots and which != "quantum":
            raise ValueError("shots apply to the quantum classifier only")
        if exact_noise:
            if which != "quantum":
                raise ValueError("exact_noise applies to the quantum classifier only")
            if shots:
                raise ValueError("exact_noise computes the expectation of the noisy device itself: it takes no shots")
            if noise is None:
                raise ValueError("exact_noise needs noise=NoiseModel(...)")
        elif noise is not None and not shots:
            raise ValueError("noise needs shots")
        clf = self.sc if which == "classical" else self.qsc
        assert clf is not None, f"no {which} classifier loaded"
        x = x.contiguous().float()
        N = x.shape[0]
        out = torch.empty(N, dtype=torch.int64, device=self.dev)
        lp = lbuf = None
        if return_logp:
            C = 3 if which == "classical" else self.qsc.C
            lp = torch.empty(N, C, device=self.dev)
            if which == "quantum":
                lbuf = self._logp.setdefault(C, torch.zeros(self.chunk, C, device=self.dev))
        for lo in range(0, N, self.chunk):
            n = min(self.chunk, N - lo)
            self._load(x, lo, n)
            if which == "classical":
                lbuf = self.sc.forward(self.xq, self.pred)
            else:
                self.qsc.infer(self.xq, self.pred, logp=lbuf, shots=shots, seed=seed, counter=lo // self.chunk,
                               noise=noise, trajectories=trajectories, valid=n, exact_noise=exact_noise)
            out[lo:lo + n].copy_(self.pred[:n])
            if return_logp:
                lp[lo:lo + n].copy_(lbuf[:n])
        return (out, lp) if return_logp else out

    @torch.no_grad()
    def estimate(self, x: torch.Tensor, expert: torch.Tensor) -> torch.Tensor:
        """Routed estimate (N, 2048) fp32: sample i through expert ``expert[i]`` and the shared FC.  Every
        expert's conv stack runs on every sample by design (see the module docstring); ``estimate_mixed`` relies
        on it: its GEMM reads all the rows (b, e) this one selects from."""
        from ..ops.fc import gemm_fwd, gemm_fwd_rows_f8
        x = x.contiguous().float()
        N = x.shape[0]
        expert = expert.to(self.dev, torch.int64)
        out = torch.empty(N, self.W_lp.shape[0], device=self.dev)
        for lo in range(0, N, self.chunk):
            n = min(self.chunk, N - lo)
            self._load(x, lo, n)
            self.pred[:n].copy_(expert[lo:lo + n])
            h = self.conv.forward(self.x1, training=False)            # (chunk * E, 32 H W) bf16, rows (b, e)
            if self.dtype == "fp8":                                   # (h: e4m3 rows, conv.rs their scales)
                gemm_fwd_rows_f8(h, self.W8, self.conv.rs, self.cs, self.b_lp, out=self.Y, cfg=self.f8_cfg,
                                 expert=self.pred, n_experts=self.E)
            else:
                gemm_fwd(h, self.W_lp, self.b_lp, out=self.Y, expert=self.pred, n_experts=self.E)
            out[lo:lo + n].copy_(self.Y[:n])
        return out

    @torch.no_grad()
    def estimate_mixed(self, x: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
        """Soft-routed estimate (N, 2048) fp32: sum_e weights[i, e] * (expert e of sample i through the shared
        FC), the combination in the FC GEMM's epilogue (ops.fc.gemm_fwd_mix; the bias is added once, so this is
        ``engine.estimate_mixed`` for weights that sum to 1).  ``weights`` (N, E) fp32, e.g. ``exp(logp)`` of
        ``classify(..., return_logp=True)``.  The chunk must be a multiple of 48 (whole GEMM tiles; ``dtype="fp8"``:
        of 144, checked at construction)."""
        from ..ops.fc import gemm_fwd_mix, gemm_fwd_mix_rows_f8
        x = x.contiguous().float()
        N = x.shape[0]
        if weights.dim() != 2 or tuple(weights.shape) != (N, self.E):
            raise ValueError(f"weights must be ({N}, {self.E}), got {tuple(weights.shape)}")
        weights = weights.to(self.dev, torch.float32)
        out = torch.empty(N, self.W_lp.shape[0], device=self.dev)
        for lo in range(0, N, self.chunk):
            n = min(self.chunk, N - lo)
            self._load(x, lo, n)
            self.wmix[:n].copy_(weights[lo:lo + n])
            if n < self.chunk:   # (the tail repeats sample lo, as _load's: its outputs are dropped)
                self.wmix[n:].copy_(weights[lo:lo + 1].expand(self.chunk - n, self.E))
            h = self.conv.forward(self.x1, training=False)            # (chunk * E, 32 H W) bf16, rows (b, e)
            if self.dtype == "fp8":
                gemm_fwd_mix_rows_f8(h, self.W8, self.conv.rs, self.cs, self.b_lp, self.wmix, out=self.Y,
                                     cfg=self.f8_cfg)
            else:
                gemm_fwd_mix(h, self.W_lp, self.b_lp, self.wmix, out=self.Y)
            out[lo:lo + n].copy_(self.Y[:n])
        return out


class InferSession:
    """One request of ``batch`` (1..16) samples from pilots to channel as ONE captured graph on one stream.

    ``which``: "quantum" / "classical" -- the engine's classifier runs in the graph and routes on the device; None:
    the caller supplies ``expert=`` (hard) or ``weights=`` (soft) to ``run``.  ``routing``: "hard" (top-1, the routed
    skinny FC reads ``pred`` in place) or "soft" (``wmix = exp(logp)`` on the device, the mixing skinny FC).  ``shots``
    / ``seed`` / ``noise`` / ``trajectories`` as ``classify`` ("quantum" only): the shot stream is keyed by ``seed`` and
    a device call counter that the graph advances by one per ``run`` (run r of a session draws what ``classify`` draws
    for chunk r), so repeated runs draw fresh shots and a fresh session with the same seed repeats the sequence.

    The session owns the static buffers (input, x1, pred, logp, wmix, Y, the skinny FC's workspace), a
    ``ConvStackHIP(model, 1, batch)`` and a classifier step at ``batch`` over the ENGINE's classifier module and flat
    space; the estimator model, W_lp, b_lp, W8 and cs are the engine's, so ``refresh`` / ``load_bn_stats`` /
    ``recalibrate_bn`` there reach the next ``run``.  No kernel of the chain needs padding at 1..16 samples, and none
    mixes samples (BN runs on its running statistics), so a sample's outputs do not depend on ``batch``.

    ``run(x)`` copies x into the static input, replays the graph and returns views of the static outputs, valid until
    the next ``run``: H (batch, 2048) bf16, pred (batch,) int64, logp (batch, C) fp32 (None when ``which`` is None;
    pred is None too for soft routing without a classifier).  No host synchronisation.  Everything refused is a
    ValueError at construction or before the replay, with nothing launched.  The graph executable follows
    utils/profiling.py's rule (``close``: parked, destroyed at exit)."""

    def __init__(self, eng: HIPInference, batch: int, which: Optional[str], routing: str, shots: int, seed: int,
                 noise, trajectories: int):
        from ..ops.conv import ConvStackHIP
        from ..ops.fc import gemm_fwd_skinny_ok, gemm_skinny_workspace
        from ..ops.qsc import QSCStepHIP
        from ..ops.quantum import resolve_measure
        from ..ops.sc import SCStepHIP
        from ..utils.profiling import GraphedStep
        if not isinstance(batch, int) or not 1 <= batch <= 16:
            raise ValueError(f"session: batch must be 1..16, got {batch!r}")
        if which not in ("quantum", "classical", None):
            raise ValueError(f"session: which must be 'quantum', 'classical' or None, got {which!r}")
        if routing not in ("hard", "soft"):
            raise ValueError(f"session: routing must be 'hard' or 'soft', got {routing!r}")
        if shots and which != "quantum":
            raise ValueError("shots apply to the quantum classifier only")
        if noise is not None and not shots:
            raise ValueError("noise needs shots")
        clf = None if which is None else (eng.sc if which == "classical" else eng.qsc)
        if which is not None and clf is None:
            raise ValueError(f"session: no {which} classifier loaded")
        self.C = None if which is None else (3 if which == "classical" else eng.qsc.C)
        if routing == "soft" and which is not None and self.C != eng.E:
            raise ValueError(f"session: soft routing needs one class per expert ({self.C} classes, {eng.E} experts)")
        if routing == "soft" and eng.E != 3:
            raise ValueError(f"session: the mixing FC takes 3 experts, the engine has {eng.E}")
        N, K = eng.W_lp.shape
        fp8 = eng.dtype == "fp8"
        if not gemm_fwd_skinny_ok(batch, N, K, fp8):
            raise ValueError(f"session: the skinny FC does not cover (N, K) = {(N, K)} (N % 16 == 0, K % 512 == 0)")
        if shots:   # (what infer would refuse, refused here and with its exception)
            resolve_measure("adjoint", shots, noise, trajectories if noise is not None else 1, None, eng.qsc.n,
                            eng.qsc.L, "hip", eng.dev)
        self.eng, self.batch, self.which, self.routing, self.fp8 = eng, batch, which, routing, fp8
        self.shots, self.seed, self.noise, self.trajectories = int(shots), int(seed), noise, trajectories
        dev = eng.dev
        self.conv = ConvStackHIP(eng.model, 1, batch)
        self.conv.rows_f8 = fp8
        self.clf = None
        if which == "classical":
            self.clf = SCStepHIP(eng._sc_mod, eng.sc.space)
        elif which == "quantum":
            self.clf = QSCStepHIP(eng._qsc_mod, eng.qsc.space, batch, n_groups=1)
        self.x = torch.zeros(batch, 2, eng.H, eng.W, device=dev)
        self.x1 = torch.zeros(batch, 2 * eng.E, eng.H, eng.W, device=dev)
        self.idx = torch.arange(batch, dtype=torch.int64, device=dev)
        self.pred = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.logp = None if which is None else torch.zeros(batch, self.C, device=dev)
        self.wmix = torch.zeros(batch, eng.E, device=dev)
        self.Y = torch.zeros(batch, N, device=dev, dtype=torch.bfloat16)
        self.ws = gemm_skinny_workspace(N, K, dev, cached=False)
        self.ctr = torch.zeros((), dtype=torch.int64, device=dev) if shots else None
        self._sc_fwd = nat.fn(nat.hip_lib(), "qd_sc_fwd", [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p,
                                                            _p]) if which == "classical" else None
        self.launches = []
        self._record = True
        self._step = GraphedStep(self._chain, warmup=1)
        with torch.no_grad():
            self._step.capture()
        if self.ctr is not None:
            self.ctr.zero_()         # (the warm-up advanced it)
        torch.cuda.current_stream(dev).synchronize()

    def _note(self, *names: str) -> None:
        if self._record:
            self.launches.extend(names)

    def _chain(self) -> None:
        """The request's launches, in order, on the current stream (captured once)."""
        from ..ops.fc import (gemm_fwd_skinny, gemm_fwd_skinny_mix, gemm_fwd_skinny_mix_rows_f8,
                              gemm_fwd_skinny_rows_f8)
        from ..ops.quantum import counter_add
        eng, st = self.eng, nat.stream_ptr(self.eng.dev)
        nat.check(eng._gather(nat.ptr(self.idx), nat.ptr(self.x), 0, nat.ptr(self.x1), None, None, 0, eng.E, 1,
                              self.batch, eng._plane, st), "gather(x1)")
        self._note("gather: x -> experts-in-channels x1")
        if self.which == "classical":
            sc = self.clf
            nat.check(self._sc_fwd(nat.ptr(self.x), nat.ptr(sc.space.flat), sc.offs, None, self.batch, sc.SPB_FWD, sc.H,
                                   sc.W, None, None, None, None, None, None, nat.ptr(self.logp), nat.ptr(self.pred), st),
                      "sc_fwd")
            self._note("sc_fwd: SC_P128 forward, log-posterior and argmax")
        elif self.which == "quantum":
            self.clf.infer(self.x, self.pred, logp=self.logp, shots=self.shots, seed=self.seed,
                           counter=self.ctr if self.ctr is not None else 0, noise=self.noise,
                           trajectories=self.trajectories)
            self._note("qsc preprocess forward", "circuit forward" + (" (measured)" if self.shots else ""),
                       "qsc head: log-posterior and argmax")
            if self.ctr is not None:
                counter_add(self.ctr, 1)
                self._note("counter += 1")
        if self.routing == "soft" and self.which is not None:
            torch.exp(self.logp, out=self.wmix)
            self._note("wmix = exp(logp)")
        h = self.conv.forward(self.x1, training=False)
        self._note("conv weight pack", "conv1", "conv2 (+ BN1)", "conv3 (+ BN2)")
        self._note(*(("BN tail", "BN3 + ReLU + e4m3 row quantisation") if self.fp8 else ("BN3 + ReLU apply with the BN tail",)))
        if self.routing == "hard":
            if self.fp8:
                gemm_fwd_skinny_rows_f8(h, eng.W8, self.conv.rs, eng.cs, eng.b_lp, out=self.Y, expert=self.pred,
                                        n_experts=eng.E, ws=self.ws)
            else:
                gemm_fwd_skinny(h, eng.W_lp, eng.b_lp, out=self.Y, expert=self.pred, n_experts=eng.E, ws=self.ws)
        elif self.fp8:
            gemm_fwd_skinny_mix_rows_f8(h, eng.W8, self.conv.rs, eng.cs, eng.b_lp, self.wmix, out=self.Y, ws=self.ws)
        else:
            gemm_fwd_skinny_mix(h, eng.W_lp, eng.b_lp, self.wmix, out=self.Y, ws=self.ws)
        self._note("skinny FC (" + ("routed" if self.routing == "hard" else "mix") + (", e4m3" if self.fp8 else ", bf16") + ")")
        self._record = False

    @torch.no_grad()
    def run(self, x: torch.Tensor, expert: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
        eng = self.eng
        if self._step is None:
            raise ValueError("session: closed")
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError(f"session: input must be {tuple(self.x.shape)}, got {tuple(x.shape)}")
        if self.which is None:
            if self.routing == "hard":
                if expert is None or tuple(expert.shape) != (self.batch,):
                    raise ValueError(f"session(which=None): run needs expert= of shape ({self.batch},)")
            elif weights is None or tuple(weights.shape) != (self.batch, eng.E):
                raise ValueError(f"session(which=None, routing='soft'): run needs weights= of shape "
                                 f"({self.batch}, {eng.E})")
        elif expert is not None or weights is not None:
            raise ValueError("session: expert= / weights= are for a session without a classifier (which=None)")
        self.x.copy_(x, non_blocking=True)
        if self.which is None:
            if self.routing == "hard":
                self.pred.copy_(expert, non_blocking=True)
            else:
                self.wmix.copy_(weights, non_blocking=True)
        self._step()
        pred = None if (self.which is None and self.routing == "soft") else self.pred
        return self.Y, pred, self.logp

    def close(self) -> None:
        """Retire the session: its graph executable is parked (utils/profiling.py) and ``run`` refuses."""
        if self._step is not None:
            self._step.close()
            self._step = None
