"""Quantum natural gradient for the QSC circuit: the block-diagonal Fubini-Study metric and its preconditioner
(csrc/hip/qsim_metric.hip; PennyLane's ``metric_tensor(approx="block-diag")`` with ``QNGOptimizer``).

Parameter p = (l n + q) 2 + k is ``w[l, q, k]``.  The metric has 2L blocks of n x n, block 2 l + k per sample:

* k = 0 (RY): g_ij = (<Y_i Y_j> - <Y_i><Y_j>) / 4 on the state that enters layer l; for l = 0 that is |0..0> and the
  block is I / 4.  Measured as a Z covariance behind RZ(pi/2) then RY(pi/2) on every wire.
* k = 1 (RZ): g_ij = (<Z_i Z_j> - <Z_i><Z_j>) / 4 on the state behind layer l's RY gates.

The Z covariance of probabilities p: m = p @ z, C = z^T diag(p) z, g = (C - m m^T) / 4 with z = ``z_signs(n)``.  The
batch metric is the mean over the step's samples, and the natural gradient of block b is (g_b + lam I)^-1 grad_b.
``hip`` (n <= 12) computes in fp32 on the GPU; ``cpu`` is the float64 oracle, a complex128 gate-by-gate walk.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from .. import _native as nat
from .quantum import _check_backend, _check_shapes, default_backend, reduce_slab, ring_inverse_index, z_signs

_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
HIP_MAX_QUBITS = 12   # csrc/hip/qsim_metric.hip: the state and its basis-changed copy in one workgroup's LDS


def _hip_limit(n: int) -> None:
    if n > HIP_MAX_QUBITS:
        raise NotImplementedError(f"the hip metric tensor supports n_qubits <= {HIP_MAX_QUBITS}, got {n}")


def _check_lambda(lam) -> float:
    lam = float(lam)
    if not (lam > 0.0 and math.isfinite(lam)):   # (NaN fails too)
        raise ValueError(f"lam must be a finite positive number, got {lam}")
    return lam


def hip_metric_rows(x: torch.Tensor, w: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Raw launcher: rows (B, 2L n n) fp32 = every sample's metric blocks; x (B, n), w (L, n, 2) fp32 contiguous."""
    B, n = x.shape
    f = nat.fn(nat.hip_lib(), "qd_qsim_metric", [_p, _p, _p, _i, _i, _i, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(rows), B, n, w.shape[0], nat.stream_ptr(x.device)), "qd_qsim_metric")
    return rows


def hip_qng_solve(gsum: torch.Tensor, B: int, lam: float, grad: torch.Tensor) -> None:
    """Raw launcher: grad (L, n, 2) fp32 contiguous, in place <- per block (gsum_b / B + lam I)^-1 grad_b."""
    L, n, _ = grad.shape
    f = nat.fn(nat.hip_lib(), "qd_qng_solve", [_p, _i, _f, _p, _i, _i, _p])
    nat.check(f(nat.ptr(gsum), B, lam, nat.ptr(grad), n, L, nat.stream_ptr(grad.device)), "qd_qng_solve")


def _rotate(state: torch.Tensor, q: int, u) -> torch.Tensor:
    """The 2 x 2 matrix u = ((u00, u01), (u10, u11)) on wire q (bit q of the index) of state (B, 2^n)."""
    B, D = state.shape
    v = state.view(B, D >> (q + 1), 2, 1 << q)
    a0, a1 = v[:, :, 0, :], v[:, :, 1, :]
    (u00, u01), (u10, u11) = u
    return torch.stack([u00 * a0 + u01 * a1, u10 * a0 + u11 * a1], dim=2).reshape(B, D)


def _ry(theta):
    c, s = torch.cos(theta / 2), torch.sin(theta / 2)
    if c.dim():   # per sample
        c, s = c.view(-1, 1, 1), s.view(-1, 1, 1)
    return (c, -s), (s, c)


def _rz(phi):
    e = torch.complex(torch.cos(phi / 2), -torch.sin(phi / 2))
    return (e, 0.0), (0.0, e.conj())


def _z_covariance(state: torch.Tensor, zs: torch.Tensor) -> torch.Tensor:
    p = state.real ** 2 + state.imag ** 2
    m = p @ zs
    C = torch.einsum("bk,ki,kj->bij", p, zs, zs)
    return 0.25 * (C - m[:, :, None] * m[:, None, :])


def _metric_cpu(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """(B, 2L, n, n) float64: the definition, gate by gate in complex128."""
    B, n = x.shape
    L = w.shape[0]
    x, w = x.double(), w.double()
    zs = z_signs(n, dtype=torch.float64)
    perm = ring_inverse_index(n)
    half_pi = torch.tensor(0.5 * math.pi, dtype=torch.float64)
    state = torch.zeros(B, 1 << n, dtype=torch.complex128)
    state[:, 0] = 1.0
    out = torch.empty(B, 2 * L, n, n, dtype=torch.float64)
    for l in range(L):
        # RY block: <Y Y> covariance of the entering state = Z covariance behind RZ(pi/2), RY(pi/2) on every wire
        t = state
        for q in range(n):
            t = _rotate(_rotate(t, q, _rz(half_pi)), q, _ry(half_pi))
        out[:, 2 * l] = _z_covariance(t, zs)
        for q in range(n):
            state = _rotate(state, q, _ry(w[l, q, 0] + x[:, q] if l == 0 else w[l, q, 0]))
        out[:, 2 * l + 1] = _z_covariance(state, zs)
        for q in range(n):
            state = _rotate(state, q, _rz(w[l, q, 1]))
        state = state[:, perm]
    return out


def metric_tensor(x: torch.Tensor, w: torch.Tensor, backend: Optional[str] = None,
                  per_sample: bool = False) -> torch.Tensor:
    """The block-diagonal Fubini-Study metric of the QSC circuit at angles x (B, n) and weights w (L, n, 2):
    (2L, n, n), the mean over the samples, or (B, 2L, n, n) with ``per_sample``.  ``hip``: fp32 on the GPU
    (n <= 12); ``cpu``: float64."""
    _check_shapes(x, w)
    if w.dim() != 3:
        raise ValueError(f"the metric is taken at the master weights (L, n, 2), got {tuple(w.shape)}")
    if x.shape[0] < 1:
        raise ValueError("the metric needs at least one sample")
    be = backend or default_backend(x.device)
    _check_backend(be, x.device)
    B, n = x.shape
    L = w.shape[0]
    if be == "hip":
        _hip_limit(n)
        rows = torch.empty(B, 2 * L * n * n, device=x.device, dtype=torch.float32)
        hip_metric_rows(x.detach().float().contiguous(), w.detach().float().contiguous(), rows)
        if per_sample:
            return rows.view(B, 2 * L, n, n)
        gsum = torch.empty(2 * L * n * n, device=x.device, dtype=torch.float32)
        return (reduce_slab(rows, gsum) / B).view(2 * L, n, n)
    if be != "cpu":
        raise ValueError(f"metric_tensor has the backends hip and cpu, not {be!r}")
    g = _metric_cpu(x.detach(), w.detach())
    return g if per_sample else g.mean(0)


class QNGPreconditioner:
    """``precondition(grad, x, w)``: the quantum layer's gradient (L, n, 2), in place, becomes the natural gradient
    (g_b + lam I)^-1 grad_b per block b = (l, k), g the mean metric over the step's samples x (B, n) at the weights w.
    On a GPU three launches on the current stream (metric rows, their deterministic row sum, the Cholesky solve) over
    workspaces the object owns: nothing is allocated inside a graph capture once the batch size has been seen.  On
    the CPU float64 ``torch.linalg.solve``, cast back to fp32."""

    def __init__(self, n: int, L: int, lam: float = 0.01, device="cpu"):
        self.n, self.L = int(n), int(L)
        if self.n < 2 or self.L < 1:
            raise ValueError(f"the circuit needs n_qubits >= 2 and n_layers >= 1, got {n} and {L}")
        self.lam = _check_lambda(lam)
        self.device = torch.device(device)
        self.rows = None
        self.gsum = None
        if self.device.type == "cuda":
            _hip_limit(self.n)
            self.gsum = torch.empty(2 * self.L * self.n * self.n, device=self.device, dtype=torch.float32)

    def reserve(self, B: int) -> None:
        """(GPU) the workspace of batches of up to B samples, ahead of a capture (it only ever grows)."""
        if self.device.type == "cuda" and (self.rows is None or self.rows.shape[0] < B):
            self.rows = torch.empty(int(B), 2 * self.L * self.n * self.n, device=self.device, dtype=torch.float32)

    @torch.no_grad()
    def precondition(self, grad: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        n, L = self.n, self.L
        if tuple(grad.shape) != (L, n, 2) or grad.dtype != torch.float32 or not grad.is_contiguous():
            raise ValueError(f"grad must be a contiguous fp32 ({L}, {n}, 2) tensor, got {tuple(grad.shape)} {grad.dtype}")
        if tuple(w.shape) != (L, n, 2) or x.dim() != 2 or x.shape[1] != n or x.shape[0] < 1:
            raise ValueError(f"bad shapes x={tuple(x.shape)} w={tuple(w.shape)} for n={n}, L={L}")
        if {grad.device.type, x.device.type, w.device.type} != {self.device.type}:
            raise ValueError(f"grad, x and w must live on {self.device.type}")
        B = x.shape[0]
        if self.device.type == "cuda":
            self.reserve(B)
            rows = self.rows[:B]
            hip_metric_rows(x.detach().float().contiguous(), w.detach().float().contiguous(), rows)
            reduce_slab(rows, self.gsum)
            hip_qng_solve(self.gsum, B, self.lam, grad)
            return grad
        g = _metric_cpu(x.detach(), w.detach()).mean(0)
        A = g + self.lam * torch.eye(n, dtype=torch.float64)
        rhs = grad.double().permute(0, 2, 1).reshape(2 * L, n, 1)
        sol = torch.linalg.solve(A, rhs).reshape(L, 2, n).permute(0, 2, 1)
        grad.copy_(sol.to(torch.float32))
        return grad
