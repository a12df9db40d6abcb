"""QuantumNAT post-measurement normalization and quantization (Wang et al., DAC 2022, sections 3.1 and 3.3): the
definition, in pure torch (any device, any float dtype, autograd).  csrc/hip/qsc_postmeas.hip's kernels are held
to this file.

The measured <Z_j> of every wire, E (B, n), are normalized over the batch per wire,

    mu_j = mean_b E[b, j]      v_j = mean_b (E[b, j] - mu_j)^2  (two passes)      z = (E - mu) rsqrt(v + eps),

which removes a per-wire affine distortion E' = c_j E + d_j -- what readout error and gate errors do to the mean of
a noisy measurement (csrc/hip/qsim_nadj.hip) -- exactly, up to eps.  The statistics go over the step's whole batch,
all streams together: the streams are not identically distributed, and a per-stream mean would subtract part of what
the head classifies on.  Training keeps running statistics by ``torch.nn.BatchNorm1d(n, affine=False)``'s rule.

With ``levels = K >= 2`` the normalized values are then snapped to K levels on [-qrange, qrange],

    D = 2 qrange / (K - 1)      Q(z) = -qrange + D rint((clamp(z, -qrange, qrange) + qrange) / D)   (ties to even),

with a straight-through backward (dy/dz = 1 where |z| <= qrange, else 0) and a quadratic penalty
sum (z - Q)^2 (Q constant in its gradient) that the loss takes as  weight * penalty_sum / (valid * n).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

STATS = ("batch", "running")


def check_quantizer(levels: int, qrange: float, weight: float = 0.0) -> None:
    if levels < 0 or levels == 1:
        raise ValueError(f"post-measurement quantization needs levels = 0 (off) or >= 2, got {levels}")
    if not qrange > 0:
        raise ValueError(f"post-measurement quantization needs qrange > 0, got {qrange}")
    if weight < 0:
        raise ValueError(f"the quantization penalty's weight must be >= 0, got {weight}")


def quantize(z: torch.Tensor, levels: int, qrange: float) -> torch.Tensor:
    """Q(z): the nearest of ``levels`` equidistant values on [-qrange, qrange] (ties to even); no gradient."""
    d = 2.0 * qrange / (levels - 1)
    with torch.no_grad():
        return -qrange + d * torch.round((z.clamp(-qrange, qrange) + qrange) / d)


def post_measurement(E: torch.Tensor, running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], *,
                     training: bool, stats: str, momentum: float = 0.1, eps: float = 1e-5, levels: int = 0,
                     qrange: float = 2.0, valid: Optional[int] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(y, z, penalty_sum) for E (B, n).  Only the first ``valid`` rows (default B) enter the batch statistics
    and the penalty; all B rows get an output.  Batch statistics when ``training`` or ``stats == "batch"``, else
    the running ones.  ``training`` also updates ``running_mean`` / ``running_var`` in place (needs valid >= 2)."""
    if stats not in STATS:
        raise ValueError(f"unknown post-measurement stats {stats!r}: one of {STATS}")
    check_quantizer(levels, qrange)
    if E.dim() != 2:
        raise ValueError(f"E must be (B, n), got {tuple(E.shape)}")
    B = E.shape[0]
    valid = B if valid is None else int(valid)
    if not 1 <= valid <= B:
        raise ValueError(f"valid must be in [1, {B}], got {valid}")
    if training and valid < 2:
        raise ValueError("post-measurement normalization trains on batch statistics: it needs at least 2 rows")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var come together")
    if running_mean is None and not training and stats == "running":
        raise ValueError("stats='running' needs running_mean and running_var")
    if training or stats == "batch":
        Ev = E[:valid]
        mu = Ev.mean(0)
        v = ((Ev - mu) ** 2).mean(0)
        if training and running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1.0 - momentum).add_(mu.detach().to(running_mean.dtype), alpha=momentum)
                running_var.mul_(1.0 - momentum).add_(v.detach().to(running_var.dtype),
                                                      alpha=momentum * valid / (valid - 1))
    else:
        mu, v = running_mean.to(E.dtype), running_var.to(E.dtype)
    z = (E - mu) * torch.rsqrt(v + eps)
    if levels == 0:
        return z, z, z.new_zeros(())
    Q = quantize(z, levels, qrange)
    inside = z.detach().abs() <= qrange
    zs = torch.where(inside, z, z.detach())
    y = Q + (zs - zs.detach())          # the value is Q exactly; the gradient passes where |z| <= qrange
    penalty = ((z[:valid] - Q[:valid]) ** 2).sum()
    return y, z, penalty
