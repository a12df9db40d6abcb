"""QOC probabilistic gradient pruning for the parameter-shift gradients (csrc/hip/qoc.hip).

An on-chip QNN pays two circuits per parameter and step.  QOC's pruning accumulates the gradient magnitudes for
``accum`` steps with every parameter measured, then for ``window`` steps measures only K = P - floor(ratio P)
parameters, sampled without replacement with probability proportional to the accumulated magnitude.  ``mask`` is
what ``qsim(shift_mask=)`` / ``QSCStepHIP(shift_mask=)`` take: the kernels read it from device memory, and
``update`` rewrites it on the device from a device-resident step counter, so the whole rule replays inside a
captured graph.  The update's integer contract is stated at the top of csrc/hip/qoc.hip; ``cpu`` runs its C++ twin
(csrc/cpu/qsim_cpu.cpp qd_cpu_qoc_update), bit-identical.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict

import torch

from .. import _native as nat

_p, _i, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
MAX_PARAMS = 4096
MAX_WINDOW = 1 << 20


class QOCPruner:
    def __init__(self, n_params: int, ratio: float, accum: int = 1, window: int = 2, seed: int = 0, device="cpu"):
        P, ratio, accum, window = int(n_params), float(ratio), int(accum), int(window)
        if not 2 <= P <= MAX_PARAMS:
            raise ValueError(f"QOC pruning supports 2..{MAX_PARAMS} parameters, got {P}")
        if not 0.0 <= ratio < 1.0:   # (NaN fails too)
            raise ValueError(f"ratio must be in [0, 1), got {ratio}")
        if not 1 <= accum <= MAX_WINDOW or not 1 <= window <= MAX_WINDOW:
            raise ValueError(f"accum and window must be in 1..{MAX_WINDOW}, got {accum} and {window}")
        self.P, self.ratio, self.accum, self.window = P, ratio, accum, window
        self.K = P - int(math.floor(ratio * P))
        if self.K < 1:
            raise ValueError(f"ratio {ratio} keeps no parameter of {P}")
        self.seed = int(seed) & ((1 << 64) - 1)
        self.device = torch.device(device)
        self.acc = torch.zeros(P, dtype=torch.float32, device=self.device)
        self.mask = torch.ones(P, dtype=torch.uint8, device=self.device)
        self.step = torch.zeros((), dtype=torch.int64, device=self.device)

    @property
    def tensors(self):
        return [self.acc, self.mask, self.step]

    @torch.no_grad()
    def update(self, grad: torch.Tensor) -> None:
        """Account this step's raw gradient (P fp32 values on the pruner's device, any shape) and write the next
        step's mask.  One launch on the current stream, graph-capturable."""
        if grad.numel() != self.P or grad.dtype != torch.float32 or grad.device.type != self.device.type:
            raise ValueError(f"grad must hold {self.P} fp32 values on {self.device.type}, got {tuple(grad.shape)} "
                             f"{grad.dtype} on {grad.device.type}")
        if not grad.is_contiguous():
            grad = grad.contiguous()
        if self.device.type == "cuda":
            f = nat.fn(nat.hip_lib(), "qd_qoc_update", [_p, _p, _p, _p, _i, _i, _i, _i, _u64, _p])
            nat.check(f(nat.ptr(self.acc), nat.ptr(self.mask), nat.ptr(self.step), nat.ptr(grad), self.P, self.accum,
                        self.window, self.K, self.seed, nat.stream_ptr(self.device)), "qd_qoc_update")
        else:
            f = nat.fn(nat.cpu_lib(), "qd_cpu_qoc_update", [_p, _p, _p, _p, _i, _i, _i, _i, _u64])
            nat.check(f(nat.ptr(self.acc), nat.ptr(self.mask), nat.ptr(self.step), nat.ptr(grad), self.P, self.accum,
                        self.window, self.K, self.seed), "qd_cpu_qoc_update")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"acc": self.acc.cpu().clone(), "mask": self.mask.cpu().clone(), "step": self.step.cpu().clone()}

    @torch.no_grad()
    def load_state_dict(self, st: Dict[str, torch.Tensor]) -> None:
        for name in ("acc", "mask", "step"):
            t = getattr(self, name)
            if tuple(st[name].shape) != tuple(t.shape):
                raise ValueError(f"pruner state {name} has shape {tuple(st[name].shape)}, expected {tuple(t.shape)}")
            t.copy_(st[name].to(t.dtype))
