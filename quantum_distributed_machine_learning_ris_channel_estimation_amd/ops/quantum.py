"""Variational-quantum-circuit layer: expectation values <Z_i> of the QSC circuit.

Reference behaviour: ``QSC_P128.qlayer`` = PennyLane ``TorchLayer`` over a
``default.qubit`` QNode (Estimators_QuantumNAT_onchipQNN.py:121-149): AngleEmbedding
RY(x_i), then per layer RY(w[l,i,0]) RZ(w[l,i,1]) on every wire and a CNOT ring,
measured as [<Z_0>, ..., <Z_{n-1}>].  PennyLane differentiates it by backprop
through its tape ("best" diff method, E:148).

Here three interchangeable backends implement the SAME function:

* ``hip``   -- hand-written CDNA4 kernels: csrc/hip/qsim.hip (n <= 10: register-resident
               state, one wave per sample) and csrc/hip/qsim_big.hip (n = 11..16: one
               512-thread workgroup per sample, state in LDS or an HBM workspace),
               forward + adjoint backward.  Default on GPU.
* ``cpu``   -- C++/OpenMP simulator (csrc/cpu/qsim_cpu.cpp). Default on CPU.
* ``torch`` -- eager complex-tensor simulator differentiated by autograd: the
               "reference-equivalent" gate-by-gate path used as a baseline and an
               oracle.  Never selected implicitly on a GPU.

Finite shots (``qsim(..., shots=N)``, ``qsim_probs``, ``sample_z``, ``counter_add``): <Z_i> estimated from N
measurement shots of the final state -- csrc/hip/qsim_shots.hip (n <= 12) and csrc/hip/qsim_stream_shots.hip (n =
13..16 with L >= 2: probabilities, sampler and the fused forward, the exact adjoint behind it) on ``hip``,
simulate-then-sample on ``cpu`` with the same integer sampling contract (``sample_z``: n <= 16 on both); by default
gradients stay the exact adjoint (straight-through).

Parameter shift (``qsim(..., diff_method="parameter_shift")``, ``pshift_rows``): the backward an on-chip QNN can
measure -- two more runs of the circuit per parameter, one angle shifted by +-pi/2, exact or with the forward's
finite shots; csrc/hip/qsim_pshift.hip (n <= 12) on ``hip``, composed from ``qsim_probs`` and ``sample_z`` on ``cpu``.

Device noise (``NoiseModel``, ``qsim(..., shots=N, noise=, trajectories=T)``, ``noise_sites``, ``pauli_frames``,
``qsim_probs(frames=)``, ``sample_z_noisy``): the shots are measured under Pauli gate errors and readout error, the
gate errors of each of T trajectories collapsed into one Pauli frame per layer -- csrc/hip/qsim_noise.hip (n <= 12)
on ``hip``, composed from the C++ oracles of the same integer contract on ``cpu``; gradients stay straight-through.

On-chip gradients (``qsim(..., shots=N, diff_method="on_chip", noise=, trajectories=T)``, ``pshift_rows(noise=)``):
the parameter-shift rule with every shifted circuit measured on that noisy device under its own counter --
csrc/hip/qsim_onchip.hip (n <= 12) on ``hip``, the noisy forward's host composition per circuit on ``cpu``.

Noise-aware adjoint (``qsim(..., shots=N, noise=, trajectories=T, diff_method="noisy_adjoint")``,
``noisy_adjoint_rows``): the exact gradient of the noisy forward's mean given its sampled Pauli frames -- the adjoint
method run through every trajectory's framed circuit, what QuantumNAT's noise injection differentiates on a
simulator; csrc/hip/qsim_nadj.hip (n <= 12) on ``hip``, the parameter-shift rule over ``qsim_probs(frames=)`` in
fp64 on ``cpu``.

The measurement arguments of all of these are validated in one place, ``resolve_measure``, into a ``MeasureMode``;
``qsim`` and the fused step (ops/qsc.py) select their kernels from it through ``hip_measured_fwd`` / ``hip_measured_rows``.

Exact noisy expectation (``qsim_mixed``, ``qsim_mixed_probs``, ``mixed_rows``; functions of their own, ``qsim`` still
refuses noise without shots): what the noisy modes above estimate -- the density matrix of the circuit under the same
Pauli channel taken in expectation, then the readout's affine map; no shots, no trajectories;
csrc/hip/qsim_mixed.hip (n <= 8) on ``hip``, the complex128 oracle of csrc/cpu/qsim_cpu.cpp on ``cpu``.  Its gradient
is the shift rule over forward launches (``mixed_rows``) or, with ``diff_method="adjoint"``, one reverse-mode launch
(``mixed_adjoint_rows``; gate rates <= 0.5).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Optional

import torch

from .. import _native as nat

_i = ctypes.c_int
_f = ctypes.c_float
_p = ctypes.c_void_p


def _opt(t: Optional[torch.Tensor]):
    return nat.ptr(t) if t is not None else None


def _check_backend(be: str, device: Optional[torch.device] = None) -> None:
    """``be`` names a backend, and (given their device) the tensors live where it computes."""
    if be not in ("hip", "cpu", "torch"):
        raise ValueError(f"unknown backend {be!r}")
    if be == "hip" and device is not None and device.type != "cuda":
        raise RuntimeError("hip backend needs CUDA/HIP tensors")
    if be == "cpu" and device is not None and device.type != "cpu":
        raise RuntimeError("cpu backend needs CPU tensors")


def reduce_slab(slab: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out (P) fp32 = the column sums of slab (rows, P) fp32, on the current stream and in a fixed order
    (deterministic: no float atomics)."""
    name = "qd_reduce_slab"
    r = nat.fn(nat.hip_lib(), name, [_p, _p, _i, _i, _f, _p])
    nat.check(r(nat.ptr(slab), nat.ptr(out), slab.shape[0], slab.shape[1], 0.0, nat.stream_ptr(slab.device)), name)
    return out

HIP_REG_MAX_QUBITS = 10   # register-resident kernel
HIP_MAX_QUBITS = 16       # workgroup-per-sample kernel above that


def stream_sim_ok(n: int, L: int) -> bool:
    """(n, L) runs on the streamed simulator (csrc/hip/qsim_stream.hip: n = 13..16, L >= 2, one
    workgroup per (sample, 4096-amplitude brick) per pass); else qsim_big.hip's workgroup-per-sample
    kernels run it."""
    return bool(nat.fn(nat.hip_lib(), "qd_qsim_stream_ok", [_i, _i])(n, L))


def _stream_ws(n: int, B: int, L: int, backward: bool, device) -> torch.Tensor:
    nbytes = nat.fn(nat.hip_lib(), "qd_qsim_stream_workspace", [_i, _i, _i, _i], ctypes.c_longlong)(n, B, L,
                                                                                                 int(backward))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _big_ws(n: int, grid: int, backward: bool, device) -> Optional[torch.Tensor]:
    nbytes = nat.fn(nat.hip_lib(), "qd_qsim_big_workspace", [_i, _i, _i], ctypes.c_longlong)(n, grid, int(backward))
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def hip_qsim_fwd(x: torch.Tensor, w: torch.Tensor, E: torch.Tensor, wgroup: int = 0) -> None:
    """Raw launcher (no autograd): E = <Z>(x, w); x (B, n) fp32, w (L, n, 2) or (G, L, n, 2) fp32."""
    lib = nat.hip_lib()
    B, n = x.shape
    L = w.shape[-3]
    st = nat.stream_ptr(x.device)
    if n <= HIP_REG_MAX_QUBITS:
        f = nat.fn(lib, "qd_qsim_fwd", [_p, _p, _p, _i, _i, _i, _i, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), B, n, L, wgroup, st), "qd_qsim_fwd")
        return
    if stream_sim_ok(n, L):
        ws = _stream_ws(n, B, L, False, x.device)
        f = nat.fn(lib, "qd_qsim_stream_fwd", [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), B, n, L, wgroup, nat.ptr(ws), None, st), "qd_qsim_stream_fwd")
        return
    grid = nat.fn(lib, "qd_qsim_big_grid", [_i])(B)
    ws = _big_ws(n, grid, False, x.device)
    f = nat.fn(lib, "qd_qsim_big_fwd", [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), B, n, L, wgroup, nat.ptr(ws) if ws is not None else None, None,
                st), "qd_qsim_big_fwd")


def hip_qsim_bwd_slab(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, dx: torch.Tensor) -> torch.Tensor:
    """Raw adjoint backward: writes dx (B, n), returns the (rows, 2nL) weight-grad slab."""
    lib = nat.hip_lib()
    B, n = x.shape
    L = w.shape[-3]
    P = 2 * n * L
    st = nat.stream_ptr(x.device)
    if n <= HIP_REG_MAX_QUBITS:
        rows = nat.fn(lib, "qd_qsim_bwd_grid", [_i, _i])(n, B)
        slab = torch.empty(rows, P, device=x.device, dtype=torch.float32)
        f = nat.fn(lib, "qd_qsim_bwd", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(dx), nat.ptr(slab), B, n, L, wgroup_of(x, w), st),
                  "qd_qsim_bwd")
        return slab
    if stream_sim_ok(n, L):
        slab = torch.empty(nat.fn(lib, "qd_qsim_stream_rows", [_i])(B), P, device=x.device, dtype=torch.float32)
        ws = _stream_ws(n, B, L, True, x.device)
        f = nat.fn(lib, "qd_qsim_stream_bwd", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(dx), nat.ptr(slab), B, n, L, wgroup_of(x, w),
                    nat.ptr(ws), None, st), "qd_qsim_stream_bwd")
        return slab
    rows = nat.fn(lib, "qd_qsim_big_grid", [_i])(B)
    slab = torch.empty(rows, P, device=x.device, dtype=torch.float32)
    ws = _big_ws(n, rows, True, x.device)
    f = nat.fn(lib, "qd_qsim_big_bwd", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(dx), nat.ptr(slab), B, n, L, wgroup_of(x, w),
                nat.ptr(ws) if ws is not None else None, None, st), "qd_qsim_big_bwd")
    return slab


def wgroup_of(x: torch.Tensor, w: torch.Tensor) -> int:
    return x.shape[0] // w.shape[0] if w.dim() == 4 else 0


# ----------------------------------------------------------------------------- HIP
class _QSimHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, wgroup: int = 0):
        B, n = x.shape
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        E = torch.empty(B, n, device=x.device, dtype=torch.float32)
        if B > 0:
            hip_qsim_fwd(x, w, E, wgroup)
        ctx.save_for_backward(x, w)
        return E

    @staticmethod
    def backward(ctx, gE: torch.Tensor):
        x, w = ctx.saved_tensors
        B, n = x.shape
        L = w.shape[-3]
        P = 2 * n * L
        gE = gE.float().contiguous()
        dx = torch.empty_like(x)
        dw = torch.zeros(P, device=x.device, dtype=torch.float32)
        if B > 0:
            reduce_slab(hip_qsim_bwd_slab(x, w, gE, dx), dw)
        dw = dw.view(L, n, 2)
        if w.dim() == 4:  # grouped (noisy) weights: every group maps back to the same master weights
            dw = _group_grad(dw, w)
        return dx, dw, None


def _group_grad(dw: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    # The slab already summed over all samples of all groups; the grouped weights are
    # (G, L, n, 2) = master + per-group noise, so d(master) = sum_g d(w_g).  Put the total
    # in group 0 and zeros elsewhere: autograd's sum over the expand/add restores it.
    out = torch.zeros_like(w)
    out[0] = dw
    return out


# ----------------------------------------------------------------------------- CPU (C++)
class _QSimCPU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor):
        lib = nat.cpu_lib()
        B, n = x.shape
        L = w.shape[0]
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        E = torch.empty(B, n, dtype=torch.float32)
        f = nat.fn(lib, "qd_cpu_qsim_fwd", [_p, _p, _p, _i, _i, _i])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), B, n, L), "qd_cpu_qsim_fwd")
        ctx.save_for_backward(x, w)
        return E

    @staticmethod
    def backward(ctx, gE: torch.Tensor):
        x, w = ctx.saved_tensors
        lib = nat.cpu_lib()
        B, n = x.shape
        L = w.shape[0]
        gE = gE.float().contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty(L, n, 2, dtype=torch.float32)
        f = nat.fn(lib, "qd_cpu_qsim_bwd", [_p, _p, _p, _p, _p, _i, _i, _i])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(dx), nat.ptr(dw), B, n, L), "qd_cpu_qsim_bwd")
        return dx, dw


# ----------------------------------------------------------------------------- torch reference
def ring_inverse_index(n: int) -> torch.Tensor:
    """idx[j] = f^-1(j) for the CNOT-ring basis map f (CNOT(0,1) ... CNOT(n-1,0))."""
    out = []
    for j in range(1 << n):
        k = j
        k ^= (k >> (n - 1)) & 1
        for i in range(n - 2, -1, -1):
            k ^= ((k >> i) & 1) << (i + 1)
        out.append(k)
    return torch.tensor(out, dtype=torch.long)


def z_signs(n: int, device=None, dtype=torch.float32) -> torch.Tensor:
    """(2^n, n) matrix of <k|Z_i|k> = +1/-1."""
    k = torch.arange(1 << n, device=device)
    bits = (k[:, None] >> torch.arange(n, device=device)[None, :]) & 1
    return (1 - 2 * bits).to(dtype)


def qsim_torch(x: torch.Tensor, w: torch.Tensor, return_probs: bool = False) -> torch.Tensor:
    """Eager gate-by-gate simulator, differentiable through autograd (complex64).  ``return_probs``: the
    (B, 2^n) outcome probabilities instead of <Z_i>."""
    B, n = x.shape
    L = w.shape[0]
    D = 1 << n
    theta = x + w[0, :, 0]
    phi = w[0, :, 1].expand(B, n)
    ch, sh = torch.cos(theta / 2), torch.sin(theta / 2)
    cp, sp = torch.cos(phi / 2), torch.sin(phi / 2)
    c0 = torch.complex(ch * cp, -ch * sp)
    c1 = torch.complex(sh * cp, sh * sp)
    state = torch.ones(B, 1, dtype=torch.complex64, device=x.device)
    for q in range(n):  # bit q becomes the most significant so far
        state = torch.cat([state * c0[:, q:q + 1], state * c1[:, q:q + 1]], dim=1)
    perm = ring_inverse_index(n).to(x.device)
    state = state[:, perm]
    for l in range(1, L):
        for q in range(n):
            th, ph = w[l, q, 0], w[l, q, 1]
            c, s = torch.cos(th / 2), torch.sin(th / 2)
            v = state.view(B, D >> (q + 1), 2, 1 << q)
            a0, a1 = v[:, :, 0, :], v[:, :, 1, :]
            e0 = torch.complex(torch.cos(ph / 2), -torch.sin(ph / 2))
            t0 = (c * a0 - s * a1) * e0
            t1 = (s * a0 + c * a1) * e0.conj()
            state = torch.stack([t0, t1], dim=2).reshape(B, D)
        state = state[:, perm]
    probs = state.real ** 2 + state.imag ** 2
    if return_probs:
        return probs
    return probs @ z_signs(n, x.device)


# ----------------------------------------------------------------------------- dispatch
def default_backend(device: torch.device) -> str:
    return "hip" if device.type == "cuda" else "cpu"


def _check_shapes(x: torch.Tensor, w: torch.Tensor) -> None:
    if x.dim() != 2 or w.dim() not in (3, 4) or w.shape[-2] != x.shape[1] or w.shape[-1] != 2:
        raise ValueError(f"bad shapes x={tuple(x.shape)} w={tuple(w.shape)}")
    if w.dim() == 4 and x.shape[0] % w.shape[0]:
        raise ValueError("batch must be a multiple of the weight-group count")
    if x.shape[1] < 2:
        raise ValueError("the CNOT ring needs n_qubits >= 2")


# ----------------------------------------------------------------------------- finite shots
HIP_SHOTS_MAX_QUBITS = 12   # csrc/hip/qsim_shots.hip: state, ring gather buffer and CDF in one workgroup's LDS
HIP_SAMPLER_MAX_QUBITS = 16  # sample_z, and with L >= 2 probabilities / plain shots: csrc/hip/qsim_stream_shots.hip
MAX_SHOTS = 1 << 20
_u64 = ctypes.c_uint64
_M64 = (1 << 64) - 1


def _check_shots(shots: int) -> int:
    shots = int(shots)
    if not 1 <= shots <= MAX_SHOTS:
        raise ValueError(f"shots must be in 1..{MAX_SHOTS}, got {shots}")
    return shots


def split_counter(counter, device):
    """(host counter, device counter pointer or None): an int is the host part; a CUDA int64 / uint64 scalar
    tensor is read by the kernel (graph replays see its current value; follow the call with counter_add)."""
    if isinstance(counter, torch.Tensor):
        if counter.device.type != "cuda" or counter.numel() != 1 or counter.dtype not in (torch.int64, torch.uint64):
            raise ValueError("a tensor counter must be a CUDA int64 / uint64 scalar")
        if device.type != "cuda":
            raise ValueError("a device counter needs the hip backend")
        return 0, nat.ptr(counter)
    return int(counter) & _M64, None


def counter_add(counter: torch.Tensor, delta: int = 1) -> None:
    """``counter += delta`` on the current stream (a one-thread kernel, graph-capturable): launch it after a
    sampling call that reads ``counter``, so that every replay of a captured graph draws fresh shots."""
    split_counter(counter, counter.device)
    f = nat.fn(nat.hip_lib(), "qd_counter_add", [_p, _u64, _p])
    nat.check(f(nat.ptr(counter), int(delta) & _M64, nat.stream_ptr(counter.device)), "qd_counter_add")


def _stream_shots_ws(name: str, dims, device) -> Optional[torch.Tensor]:
    """The workspace of a streamed finite-shot entry point (csrc/hip/qsim_stream_shots.hip), sized by its
    ``<name>_workspace(*dims)``; None outside the entry point's range (it then refuses the call)."""
    nbytes = nat.fn(nat.hip_lib(), name + "_workspace", [_i] * len(dims), ctypes.c_longlong)(*dims)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def hip_qsim_probs(x: torch.Tensor, w: torch.Tensor, probs: torch.Tensor, wgroup: int = 0) -> None:
    """Raw launcher: probs (B, 2^n) fp32 = |amp_k|^2 in natural basis order; n <= 12 (csrc/hip/qsim_shots.hip), or
    n = 13..16 with L >= 2 on the streamed simulator (csrc/hip/qsim_stream.hip's probabilities pass)."""
    B, n = x.shape
    if n > HIP_SHOTS_MAX_QUBITS:
        name, L = "qd_qsim_stream_probs", w.shape[-3]
        ws = _stream_shots_ws(name, (n, B, L), x.device)
        f = nat.fn(nat.hip_lib(), name, [_p, _p, _p, _i, _i, _i, _i, _p, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(probs), B, n, L, wgroup, _opt(ws), nat.stream_ptr(x.device)), name)
        return
    f = nat.fn(nat.hip_lib(), "qd_qsim_probs", [_p, _p, _p, _i, _i, _i, _i, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(probs), B, n, w.shape[-3], wgroup, nat.stream_ptr(x.device)),
              "qd_qsim_probs")


def hip_sample_z(probs: torch.Tensor, E: torch.Tensor, counts: Optional[torch.Tensor], n: int, shots: int,
                 seed: int = 0, ctr0: int = 0, counter_ptr=None) -> None:
    """Raw launcher: E (B, n) fp32 / counts (B, n) int32 (nullable) from `shots` draws of every row of probs; above
    12 qubits (to 16) the block sampler of csrc/hip/qsim_stream_shots.hip."""
    if n > HIP_SHOTS_MAX_QUBITS:
        name, B = "qd_stream_sample_z", probs.shape[0]
        ws = _stream_shots_ws(name, (n, B), probs.device)
        f = nat.fn(nat.hip_lib(), name, [_p, _p, _p, _i, _i, _i, _u64, _u64, _p, _p, _p])
        nat.check(f(nat.ptr(probs), nat.ptr(E), _opt(counts), B, n, shots, seed & _M64, ctr0 & _M64, counter_ptr,
                    _opt(ws), nat.stream_ptr(probs.device)), name)
        return
    f = nat.fn(nat.hip_lib(), "qd_sample_z", [_p, _p, _p, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(probs), nat.ptr(E), _opt(counts), probs.shape[0], n, shots, seed & _M64, ctr0 & _M64,
                counter_ptr, nat.stream_ptr(probs.device)), "qd_sample_z")


def hip_qsim_shots_fwd(x: torch.Tensor, w: torch.Tensor, E: torch.Tensor, counts: Optional[torch.Tensor], shots: int,
                       seed: int = 0, ctr0: int = 0, counter_ptr=None, wgroup: int = 0) -> None:
    """Raw launcher of the fused finite-shot forward: state -> probabilities -> shots in one launch (n <= 12), or
    the streamed forward's passes, its probabilities pass and the block sampler (n = 13..16, L >= 2); only E / counts
    leave the kernels' workspace."""
    B, n = x.shape
    if n > HIP_SHOTS_MAX_QUBITS:
        name, L = "qd_qsim_stream_shots_fwd", w.shape[-3]
        ws = _stream_shots_ws(name.replace("_fwd", ""), (n, B, L), x.device)
        f = nat.fn(nat.hip_lib(), name, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _u64, _u64, _p, _p, _p])
        nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), _opt(counts), B, n, L, wgroup, shots, seed & _M64,
                    ctr0 & _M64, counter_ptr, _opt(ws), nat.stream_ptr(x.device)), name)
        return
    f = nat.fn(nat.hip_lib(), "qd_qsim_shots_fwd", [_p, _p, _p, _p, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), _opt(counts), B, n, w.shape[-3], wgroup, shots, seed & _M64,
                ctr0 & _M64, counter_ptr, nat.stream_ptr(x.device)), "qd_qsim_shots_fwd")


def _hip_shots_limit(n: int) -> None:
    if n > HIP_SHOTS_MAX_QUBITS:
        raise NotImplementedError(f"the HIP finite-shot kernels support n <= {HIP_SHOTS_MAX_QUBITS} qubits, got {n}")


def _hip_stream_shots_limit(n: int, L: int) -> None:
    """The range of the plain finite-shot kernels (probabilities, sampler, fused forward): n <= 12, and n = 13..16
    with L >= 2 on the streamed simulator; every other measured kernel stops at ``_hip_shots_limit``."""
    if not (n > HIP_SHOTS_MAX_QUBITS and stream_sim_ok(n, L)):
        _hip_shots_limit(n)


@torch.no_grad()
def qsim_probs(x: torch.Tensor, w: torch.Tensor, backend: Optional[str] = None,
               frames: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Outcome probabilities |amp_k|^2 of the QSC circuit, (B, 2^n) in natural basis order (the ``qml.probs``
    counterpart): fp32 on ``hip`` (n <= 12, or n = 13..16 with L >= 2), fp64 on ``cpu``, the eager simulator's on
    ``torch``.  No autograd.

    ``frames`` ((B, L, 2) int32, ``cpu`` only: the oracle of csrc/hip/qsim_noise.hip): row b's Pauli frames
    (a, b), applied behind the rings of layers 0 .. L-2; the last layer's frame acts on the outcome and is
    left out."""
    _check_shapes(x, w)
    B, n = x.shape
    be = backend if backend not in (None, "auto") else default_backend(x.device)
    if frames is not None:
        return _qsim_probs_framed(x, w, be, frames)
    _check_backend(be, x.device)
    if be == "hip":
        _hip_stream_shots_limit(n, w.shape[-3])
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        probs = torch.empty(B, 1 << n, device=x.device, dtype=torch.float32)
        if B > 0:
            hip_qsim_probs(x, w, probs, wgroup_of(x, w))
        return probs
    if w.dim() == 4:  # host backends: run per group
        return torch.cat([qsim_probs(xc, w[g], be) for g, xc in enumerate(x.chunk(w.shape[0]))], dim=0)
    if be == "torch":
        return qsim_torch(x, w, return_probs=True)
    x = x.detach().float().contiguous()
    w = w.detach().float().contiguous()
    probs = torch.empty(B, 1 << n, dtype=torch.float64)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_qsim_probs", [_p, _p, _p, _i, _i, _i])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(probs), B, n, w.shape[0]), "qd_cpu_qsim_probs")
    return probs


@torch.no_grad()
def sample_z(probs: torch.Tensor, shots: int, seed: int = 0, counter=0, return_counts: bool = False):
    """Finite-shot <Z_i> from outcome probabilities (B, 2^n), a normalised distribution per row (cast to fp32):
    E (B, n) fp32, and with ``return_counts`` also counts (B, n) int32, the shots that read 1 on wire i.

    Dispatches on the tensor's device: csrc/hip/qsim_shots.hip (above 12 qubits csrc/hip/qsim_stream_shots.hip) on
    the GPU, the sequential C++ sampler on the host -- the same integer contract (Philox4x32-10 keyed by ``seed``,
    counter (shot / 4, row, counter)), so the two agree bit for bit on the same fp32 probabilities.  2 <= n <= 16."""
    shots = _check_shots(shots)
    if probs.dim() != 2 or probs.shape[1] < 4 or probs.shape[1] & (probs.shape[1] - 1):
        raise ValueError(f"probs must be (B, 2^n) with n >= 2, got {tuple(probs.shape)}")
    B, n = probs.shape[0], probs.shape[1].bit_length() - 1
    if n > HIP_SAMPLER_MAX_QUBITS:   # (the host sampler keeps the kernels' range: one contract)
        raise NotImplementedError(f"the shot samplers support n <= {HIP_SAMPLER_MAX_QUBITS} qubits, got {n}")
    probs = probs.detach().float().contiguous()
    ctr0, cptr = split_counter(counter, probs.device)
    E = torch.empty(B, n, device=probs.device, dtype=torch.float32)
    counts = torch.empty(B, n, device=probs.device, dtype=torch.int32)
    if B > 0 and probs.device.type == "cuda":
        hip_sample_z(probs, E, counts, n, shots, int(seed), ctr0, cptr)
    elif B > 0:
        name = "qd_cpu_sample_z" if n <= HIP_SHOTS_MAX_QUBITS else "qd_cpu_sample_z_wide"   # (one body, two ranges)
        f = nat.fn(nat.cpu_lib(), name, [_p, _p, _p, _i, _i, _i, _u64, _u64])
        nat.check(f(nat.ptr(probs), nat.ptr(E), nat.ptr(counts), B, n, shots, int(seed) & _M64, ctr0), name)
    return (E, counts) if return_counts else E


class _ReplaceValue(torch.autograd.Function):
    """value, with the gradient handed to `exact` unchanged (straight-through)."""

    @staticmethod
    def forward(ctx, exact, value):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


# ----------------------------------------------------------------------------- Pauli noise
MAX_TRAJECTORIES = 1024
MAX_NOISE_SITES = 4096   # 2 n L


class NoiseModel:
    """Gate and readout noise of a device, for ``qsim(shots=, noise=)`` (csrc/hip/qsim_noise.hip).

    Every argument is a float or a length-n sequence, a probability in [0, 0.5]:
    ``p1[q]``: a uniformly drawn X / Y / Z after wire q's fused RZ.RY of every layer;
    ``p2[q]``: a uniformly drawn non-identity two-qubit Pauli after every CNOT whose control is wire q;
    ``readout01[i]`` / ``readout10[i]``: wire i reads 1 given 0 / 0 given 1.

    The kernels compare integers: ``thresholds(n, device)`` gives thr = min(rint(p 2^32), 2^32 - 1) for the gates
    (uint32 bits in int32 tensors) and thr16 = min(rint(r 2^16), 65535) for the readout ((n, 2) int32), computed
    in float64 on the host and cached per (n, device)."""

    FIELDS = ("p1", "p2", "readout01", "readout10")

    def __init__(self, p1=0.0, p2=0.0, readout01=0.0, readout10=0.0):
        import numpy as np
        for name, v in zip(self.FIELDS, (p1, p2, readout01, readout10)):
            a = np.atleast_1d(np.asarray(v, dtype=np.float64))
            if a.ndim != 1 or a.size < 1 or not np.all((a >= 0.0) & (a <= 0.5)):   # (NaN fails too)
                raise ValueError(f"{name} must be a probability in [0, 0.5] or a sequence of them, got {v!r}")
            setattr(self, name, a if a.size > 1 else float(a[0]))
        self._cache = {}

    def _per_wire(self, name: str, n: int):
        import numpy as np
        v = getattr(self, name)
        if isinstance(v, float):
            return np.full(n, v, dtype=np.float64)
        if v.size != n:
            raise ValueError(f"{name} has {v.size} entries for {n} wires")
        return v

    @property
    def is_zero(self) -> bool:
        import numpy as np
        return all(not np.any(np.asarray(getattr(self, f))) for f in self.FIELDS)

    def thresholds_host(self, n: int):
        """(thr1 (n) uint32, thr2 (n) uint32, thr_ro (n, 2) uint32) as NumPy arrays."""
        import numpy as np
        gate = lambda p: np.minimum(np.rint(p * 4294967296.0), 4294967295.0).astype(np.uint32)   # noqa: E731
        ro = lambda r: np.minimum(np.rint(r * 65536.0), 65535.0).astype(np.uint32)   # noqa: E731
        thr_ro = np.stack([ro(self._per_wire("readout01", n)), ro(self._per_wire("readout10", n))], axis=1)
        return gate(self._per_wire("p1", n)), gate(self._per_wire("p2", n)), np.ascontiguousarray(thr_ro)

    def thresholds(self, n: int, device) -> tuple:
        device = torch.device(device)
        key = (n, device.type, device.index)
        if key not in self._cache:
            self._cache[key] = tuple(torch.from_numpy(t.view("int32").copy()).to(device)
                                     for t in self.thresholds_host(n))
        return self._cache[key]

    def __repr__(self) -> str:
        return "NoiseModel(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in self.FIELDS) + ")"


def _check_trajectories(T, shots: Optional[int] = None) -> int:
    """T in range, and (with ``shots``) the shots split evenly over the trajectories."""
    T = int(T)
    if not 1 <= T <= MAX_TRAJECTORIES:
        raise ValueError(f"trajectories must be in 1..{MAX_TRAJECTORIES}, got {T}")
    if shots is None:
        return T
    if shots % T:
        raise ValueError(f"shots ({shots}) must be a multiple of trajectories ({T})")
    if T > 1 and (shots // T) % 4:
        raise ValueError(f"with trajectories > 1, shots / trajectories must be a multiple of 4, got {shots // T}")
    return T


def _check_noise_shape(n: int, L: int) -> None:
    if 2 * n * L > MAX_NOISE_SITES:
        raise ValueError(f"the noise model supports 2 n L <= {MAX_NOISE_SITES} error sites, got n={n} L={L}")


def _noise_qubit_limit(n: int) -> None:
    if n > HIP_SHOTS_MAX_QUBITS:   # (the host oracles keep the kernels' range: one contract)
        raise NotImplementedError(f"the noise model supports n <= {HIP_SHOTS_MAX_QUBITS} qubits, got {n}")


def _check_noise_model(noise) -> None:
    if not isinstance(noise, NoiseModel):
        raise ValueError(f"noise must be a NoiseModel, got {type(noise).__name__}")


@torch.no_grad()
def noise_sites(noise: NoiseModel, B: int, n: int, L: int, T: int = 1, seed: int = 0, counter: int = 0,
                device=None) -> torch.Tensor:
    """The error code drawn at every site of every trajectory, (B, T, L, n, 2) uint8: [..., q, 0] after wire q's
    RZ.RY (0 none, 1 / 2 / 3 = X / Y / Z), [..., q, 1] after CNOT(q, q+1) (0 none, else 4 P_control + P_target).
    Drawn on the host by the C++ oracle of the kernel's contract."""
    _check_noise_shape(n, L)
    _check_trajectories(T)
    _noise_qubit_limit(n)
    thr1, thr2, _ = noise.thresholds(n, "cpu")
    sites = torch.zeros(B, T, L, n, 2, dtype=torch.uint8)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_noise_sites", [_p, _p, _p, _i, _i, _i, _i, _u64, _u64])
    nat.check(f(nat.ptr(sites), nat.ptr(thr1), nat.ptr(thr2), B, n, L, int(T), int(seed) & _M64, int(counter) & _M64),
              "qd_cpu_noise_sites")
    return sites.to(device) if device is not None else sites


@torch.no_grad()
def pauli_frames(sites: torch.Tensor) -> torch.Tensor:
    """Site codes (..., L, n, 2) uint8 -> every layer's Pauli frame (..., L, 2) int32 = (X mask a, Z mask b)
    behind that layer's CNOT ring."""
    if sites.dim() < 3 or sites.shape[-1] != 2 or sites.dtype != torch.uint8:
        raise ValueError(f"sites must be (..., L, n, 2) uint8, got {tuple(sites.shape)} {sites.dtype}")
    L, n = sites.shape[-3], sites.shape[-2]
    _check_noise_shape(n, L)
    host = sites.detach().cpu().contiguous()
    rows = host.numel() // (2 * n * L)
    frames = torch.zeros(*sites.shape[:-3], L, 2, dtype=torch.int32)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_pauli_frames", [_p, _p, _i, _i, _i])
    nat.check(f(nat.ptr(host), nat.ptr(frames), rows, n, L), "qd_cpu_pauli_frames")
    return frames.to(sites.device)


def _qsim_probs_framed(x: torch.Tensor, w: torch.Tensor, be: str, frames: torch.Tensor) -> torch.Tensor:
    B, n = x.shape
    L = w.shape[-3]
    if be != "cpu":
        raise ValueError("qsim_probs(frames=) is the host oracle: backend 'cpu' only")
    _check_backend(be, x.device)
    if tuple(frames.shape) != (B, L, 2) or frames.dtype != torch.int32:
        raise ValueError(f"frames must be ({B}, {L}, 2) int32, got {tuple(frames.shape)} {frames.dtype}")
    _check_noise_shape(n, L)
    if w.dim() == 4:
        G = w.shape[0]
        return torch.cat([_qsim_probs_framed(xc, w[g], be, fc) for g, (xc, fc) in
                          enumerate(zip(x.chunk(G), frames.chunk(G)))], dim=0)
    x = x.detach().float().contiguous()
    w = w.detach().float().contiguous()
    frames = frames.detach().cpu().contiguous()
    probs = torch.empty(B, 1 << n, dtype=torch.float64)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_qsim_probs_framed", [_p, _p, _p, _p, _i, _i, _i])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(frames), nat.ptr(probs), B, n, L), "qd_cpu_qsim_probs_framed")
    return probs


@torch.no_grad()
def sample_z_noisy(probs: torch.Tensor, amask: torch.Tensor, noise: NoiseModel, shots: int, seed: int = 0,
                   counter: int = 0, return_counts: bool = False):
    """The host oracle of the noisy sampler: probs (B, T, 2^n) (cast to fp32), one distribution per trajectory;
    amask (B, T) int32, the X mask of each trajectory's last-layer frame; readout error from ``noise``.
    Trajectory tau owns shots [tau shots/T, (tau+1) shots/T).  E (B, n) fp32 (and counts (B, n) int32)."""
    shots = _check_shots(shots)
    if probs.dim() != 3 or probs.shape[2] < 4 or probs.shape[2] & (probs.shape[2] - 1):
        raise ValueError(f"probs must be (B, T, 2^n) with n >= 2, got {tuple(probs.shape)}")
    B, T, n = probs.shape[0], probs.shape[1], probs.shape[2].bit_length() - 1
    _check_trajectories(T, shots)
    if n > HIP_SHOTS_MAX_QUBITS:
        raise NotImplementedError(f"the shot samplers support n <= {HIP_SHOTS_MAX_QUBITS} qubits, got {n}")
    if tuple(amask.shape) != (B, T):
        raise ValueError(f"amask must be ({B}, {T}), got {tuple(amask.shape)}")
    probs = probs.detach().cpu().float().contiguous()
    amask = amask.detach().cpu().to(torch.int32).contiguous()
    thr_ro = noise.thresholds(n, "cpu")[2]
    E = torch.empty(B, n, dtype=torch.float32)
    counts = torch.empty(B, n, dtype=torch.int32)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_sample_z_noisy", [_p, _p, _p, _p, _p, _i, _i, _i, _i, _u64, _u64])
    nat.check(f(nat.ptr(probs), nat.ptr(amask), nat.ptr(thr_ro), nat.ptr(E), nat.ptr(counts), B, n, shots, T,
                int(seed) & _M64, int(counter) & _M64), "qd_cpu_sample_z_noisy")
    return (E, counts) if return_counts else E


def hip_qsim_noisy_shots_fwd(x: torch.Tensor, w: torch.Tensor, E: torch.Tensor, counts: Optional[torch.Tensor],
                             noise: NoiseModel, shots: int, trajectories: int = 1, seed: int = 0, ctr0: int = 0,
                             counter_ptr=None, wgroup: int = 0, probs_out: Optional[torch.Tensor] = None,
                             frames_out: Optional[torch.Tensor] = None) -> None:
    """Raw launcher of csrc/hip/qsim_noise.hip (n <= 12): E (B, n) fp32 / counts (B, n) int32 (nullable) of
    ``shots`` noisy shots per sample over ``trajectories`` error realisations; probs_out (nullable; B, T, 2^n)
    fp32 the probabilities each trajectory's CDF was quantised from, frames_out (nullable; B, T, L, 2) int32."""
    B, n = x.shape
    thr1, thr2, thr_ro = noise.thresholds(n, x.device)
    f = nat.fn(nat.hip_lib(), "qd_qsim_noisy_shots_fwd",
               [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(E), _opt(counts), _opt(probs_out), _opt(frames_out), nat.ptr(thr1),
                nat.ptr(thr2), nat.ptr(thr_ro), B, n, w.shape[-3], wgroup, shots, int(trajectories), seed & _M64,
                ctr0 & _M64, counter_ptr, nat.stream_ptr(x.device)), "qd_qsim_noisy_shots_fwd")


def noise_split(trajectories: int, n: int) -> int:
    """The workgroups per sample the noisy kernel launches for that many trajectories of n qubits (1: one per sample; else one
    per (sample, chunk of trajectories), the counts meeting through integer atomics: the result does not depend
    on it)."""
    return nat.fn(nat.hip_lib(), "qd_qsim_noise_split", [_i, _i])(int(trajectories), int(n))


def noise_force_split(nsplit: int) -> None:
    """Tests and timing: launch ``nsplit`` (1, 2, 4 or 8; it must divide ``trajectories``) workgroups per sample
    from now on; 0 hands the choice back to the launcher."""
    nat.check(nat.fn(nat.hip_lib(), "qd_qsim_noise_force_split", [_i])(int(nsplit)), "qd_qsim_noise_force_split")


@torch.no_grad()
def _noisy_shots_cpu(x, w, noise, shots, T, seed, ctr0) -> torch.Tensor:
    """The noisy forward composed from the host oracles: sites -> frames -> framed probabilities -> sampler."""
    B, n = x.shape
    L = w.shape[-3]
    frames = pauli_frames(noise_sites(noise, B, n, L, T, seed, ctr0))
    probs = qsim_probs(x.repeat_interleave(T, dim=0), w, "cpu", frames=frames.view(B * T, L, 2))
    return sample_z_noisy(probs.view(B, T, 1 << n), frames[:, :, L - 1, 0], noise, shots, seed, ctr0)


# ----------------------------------------------------------------------------- the measurement mode
DIFF_METHODS = ("adjoint", "parameter_shift", "on_chip", "noisy_adjoint")
_MASK_METHODS = "shift_mask needs diff_method='parameter_shift' or 'on_chip'"


@dataclasses.dataclass(frozen=True)
class MeasureMode:
    """The validated measurement arguments of a ``qsim`` call or a fused step: what ``resolve_measure`` returns
    and the shared launchers (``hip_measured_fwd``, ``hip_measured_rows``) select their kernel by."""
    diff_method: str = "adjoint"
    shots: Optional[int] = None             # None: exact expectations
    noise: Optional[NoiseModel] = None
    trajectories: int = 1
    masked: bool = False                    # a shift_mask was given


def resolve_measure(diff_method, shots, noise, trajectories, shift_mask, n: int, L: int, be: str, device,
                    mask_shape: bool = True) -> MeasureMode:
    """The one place of the measurement arguments' rules (``qsim``'s docstring states them): the mode of a circuit
    of ``n`` qubits and ``L`` layers on backend ``be`` with its tensors on ``device``, or the refusal -- first the
    rules that hold on every backend, then what the backend and its kernels support.  ``mask_shape=False`` (the
    fused step, whose mask is the kernel's flat one) leaves the shape of ``shift_mask`` to the caller.  The exact
    mode (no shots, ``"adjoint"``) is every backend's: its caller checks the backend."""
    if diff_method not in DIFF_METHODS:
        raise ValueError(f"unknown diff_method {diff_method!r}: one of {DIFF_METHODS}")
    pshift = diff_method in ("parameter_shift", "on_chip")
    T = 1
    if noise is not None:
        _check_noise_model(noise)
        if not shots:
            raise ValueError("noise needs shots: the noise model is sampled per measurement shot")
        if diff_method == "parameter_shift":
            raise ValueError("noise with diff_method='parameter_shift' is not supported: "
                             "diff_method='on_chip' measures the shifted circuits under the noise")
        if shift_mask is not None and not pshift:
            raise ValueError(_MASK_METHODS)
        shots = _check_shots(shots)
        T = _check_trajectories(trajectories, shots)
    elif int(trajectories) != 1:
        raise ValueError("trajectories needs noise")
    if diff_method == "noisy_adjoint" and noise is None:
        raise ValueError("diff_method='noisy_adjoint' needs noise= and shots=: it differentiates through the error "
                         "gates the noisy shots forward samples")
    if pshift:
        if be == "torch":
            raise ValueError("the torch backend has no parameter-shift rule; use hip or cpu")
        _check_backend(be)
        if diff_method == "on_chip" and not shots:
            raise ValueError("diff_method='on_chip' needs shots: a device measures every circuit with finite shots")
        if be == "hip" and device.type == "cuda":
            _hip_shots_limit(n)
        if 4 * n * L + 1 >= 1 << 16:
            raise ValueError(f"parameter shift needs 2 * (2 n L) + 1 < 2^16 stream ids, got n={n} L={L}")
        if shift_mask is not None and mask_shape and tuple(shift_mask.shape) != (L, n, 2):
            raise ValueError(f"shift_mask must be {(L, n, 2)}, got {tuple(shift_mask.shape)}")
        shots = _check_shots(shots) if shots else None
        if noise is not None:
            _check_noise_shape(n, L)
        _check_backend(be, device)
        return MeasureMode(diff_method, shots, noise, T, shift_mask is not None)
    if shift_mask is not None:
        raise ValueError(_MASK_METHODS)
    shots = _check_shots(shots) if shots else None
    if shots is not None:
        if be == "torch":
            raise ValueError("the torch backend has no noise model; use hip or cpu" if noise is not None else
                             "the torch backend has no finite-shot sampler; use hip or cpu")
        _check_backend(be, device)
        if be == "hip" and noise is None:   # plain shots: also the streamed simulator's sizes
            _hip_stream_shots_limit(n, L)
        elif be == "hip":
            _hip_shots_limit(n)
        if noise is not None:
            _check_noise_shape(n, L)
    return MeasureMode(diff_method, shots, noise, T, False)


def hip_measured_fwd(x: torch.Tensor, w: torch.Tensor, E: torch.Tensor, mode: MeasureMode, seed: int = 0,
                     ctr0: int = 0, counter_ptr=None, wgroup: int = 0) -> None:
    """The measured forward of a mode with shots, E (B, n) fp32: the noisy kernel under ``mode.noise``, else the
    fused finite-shot one (above 12 qubits the streamed simulator's: ``hip_qsim_shots_fwd`` picks it).  ``qsim`` and
    the fused step (ops/qsc.py) both launch through here."""
    if mode.noise is not None:
        hip_qsim_noisy_shots_fwd(x, w, E, None, mode.noise, mode.shots, mode.trajectories, seed, ctr0, counter_ptr,
                                 wgroup)
    else:
        hip_qsim_shots_fwd(x, w, E, None, mode.shots, seed, ctr0, counter_ptr, wgroup)


@torch.no_grad()
def _measured_fwd(x, w, be, mode: MeasureMode, seed, ctr0, cptr=None) -> torch.Tensor:
    """E (B, n) fp32 of a mode with shots on ``hip`` or ``cpu``; x, w fp32 contiguous."""
    if be == "hip":
        E = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        if x.shape[0] > 0:
            hip_measured_fwd(x, w, E, mode, seed, ctr0, cptr, wgroup_of(x, w))
        return E
    if mode.noise is not None:
        return _noisy_shots_cpu(x, w, mode.noise, mode.shots, mode.trajectories, seed, ctr0)
    return sample_z(qsim_probs(x, w, "cpu"), mode.shots, seed, ctr0)


class _QSimMeasuredHIP(torch.autograd.Function):
    """Forward: the finite-shot kernel, noisy or not.  Backward: the exact adjoint of the noiseless circuit (gate,
    readout and shot noise are straight-through)."""

    @staticmethod
    def forward(ctx, x, w, mode, seed, ctr0, cptr):
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        ctx.save_for_backward(x, w)
        return _measured_fwd(x, w, "hip", mode, seed, ctr0, cptr)

    @staticmethod
    def backward(ctx, gE):
        dx, dw, _ = _QSimHIP.backward(ctx, gE)
        return dx, dw, None, None, None, None


# ----------------------------------------------------------------------------- parameter shift
PSHIFT_ID_SHIFT = 48   # circuit (p, s) draws under call counter c + (id << 48), id = 1 + 2p + s; the forward is id 0


def pshift_counter(counter: int, p: int, s: int) -> int:
    """The call counter of shifted circuit (p, s) (s = 0: +pi/2, 1: -pi/2) of a call with counter ``counter``.
    Distinct from the forward's and from every other circuit's for counters below 2^48."""
    return (int(counter) + ((1 + 2 * p + s) << PSHIFT_ID_SHIFT)) & _M64


def _mask_u8(shift_mask, w: torch.Tensor) -> Optional[torch.Tensor]:
    """The kernels' flat (2nL) uint8 mask of an (L, n, 2) ``shift_mask`` (its shape: ``resolve_measure``)."""
    if shift_mask is None:
        return None
    return (shift_mask != 0).to(device=w.device, dtype=torch.uint8).reshape(-1).contiguous()


def hip_qsim_pshift(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, G: torch.Tensor,
                    Epm: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None,
                    mask: Optional[torch.Tensor] = None, need_dx: bool = True, shots: int = 0, seed: int = 0,
                    ctr0: int = 0, counter_ptr=None, wgroup: int = 0) -> None:
    """Raw launcher of csrc/hip/qsim_pshift.hip (n <= 12): G (B, P) fp32 = sum_j gE[b, j] (E+_j - E-_j) / 2 for
    every parameter p = (l n + q) 2 + k, P = 2nL; Epm (nullable; B, P, 2, n) the shifted expectations, probs
    (nullable; B, P, 2, 2^n) the probabilities they were measured from; mask (nullable; P) uint8, 0 = skip the
    parameter (a layer-0 RY one still runs with ``need_dx``).  shots = 0: exact expectations."""
    B, n = x.shape
    f = nat.fn(nat.hip_lib(), "qd_qsim_pshift",
               [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(G), _opt(Epm), _opt(probs), _opt(mask), B, n, w.shape[-3],
                wgroup, int(need_dx), shots, seed & _M64, ctr0 & _M64, counter_ptr, nat.stream_ptr(x.device)),
              "qd_qsim_pshift")


def hip_qsim_noisy_pshift(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, G: torch.Tensor,
                          Epm: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None,
                          mask: Optional[torch.Tensor] = None, need_dx: bool = True, shots: int = 0, seed: int = 0,
                          ctr0: int = 0, counter_ptr=None, wgroup: int = 0, noise: Optional["NoiseModel"] = None,
                          trajectories: int = 1, frames: Optional[torch.Tensor] = None) -> None:
    """Raw launcher of csrc/hip/qsim_onchip.hip (n <= 12): ``hip_qsim_pshift`` with every shifted circuit measured
    under ``noise`` over ``trajectories`` error realisations drawn under the circuit's own counter.  probs
    (nullable) is (B, P, 2, T, 2^n) here, frames (nullable; B, P, 2, T, L, 2) int32 every trajectory's Pauli frames."""
    B, n = x.shape
    thr1, thr2, thr_ro = (noise if noise is not None else NoiseModel()).thresholds(n, x.device)
    f = nat.fn(nat.hip_lib(), "qd_qsim_noisy_pshift",
               [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(G), _opt(Epm), _opt(probs), _opt(frames), _opt(mask),
                nat.ptr(thr1), nat.ptr(thr2), nat.ptr(thr_ro), B, n, w.shape[-3], wgroup, int(need_dx), shots,
                int(trajectories), seed & _M64, ctr0 & _M64, counter_ptr, nat.stream_ptr(x.device)),
              "qd_qsim_noisy_pshift")


def _pshift_rows_cpu(x, w, gE, mask, need_dx, shots, seed, ctr0, noise=None, T=1) -> torch.Tensor:
    """The kernel's G composed from the host oracles: qsim_probs (fp64) of the shifted weights, then sample_z under
    the circuit's counter, or the probability-weighted sum in exact mode.  With ``noise``: the noisy forward's
    composition (sites -> frames -> framed probabilities -> noisy sampler), all under the circuit's counter."""
    B, n = x.shape
    P = 2 * n * w.shape[-3]
    zs = z_signs(n, dtype=torch.float64)
    g64 = gE.double()
    G = torch.zeros(B, P, dtype=torch.float32)
    for p in range(P):
        if mask is not None and not mask[p] and not (need_dx and p < 2 * n and p % 2 == 0):
            continue
        E = []
        for s, sh in enumerate((0.5 * math.pi, -0.5 * math.pi)):
            ws = w.clone()
            ws.view(-1, P)[:, p] += sh
            if noise is not None:
                E.append(_noisy_shots_cpu(x, ws, noise, shots, T, seed, pshift_counter(ctr0, p, s)).double())
                continue
            pr = qsim_probs(x, ws, "cpu")
            E.append(sample_z(pr, shots, seed, pshift_counter(ctr0, p, s)).double() if shots else pr @ zs)
        G[:, p] = (g64 * (E[0] - E[1]) * 0.5).sum(1).float()
    return G


@torch.no_grad()
def pshift_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, backend: Optional[str] = None,
                shots: Optional[int] = None, seed: int = 0, counter=0, shift_mask: Optional[torch.Tensor] = None,
                need_dx: bool = True, noise: Optional["NoiseModel"] = None, trajectories: int = 1) -> torch.Tensor:
    """Per-sample parameter-shift gradients G (B, 2nL) fp32 of sum(gE * qsim(x, w)): column p = (l n + q) 2 + k
    is w[l, q, k]'s.  dx = G[:, 0:2n:2]; dw = G summed over the samples.  Arguments as for ``qsim``.  With
    ``noise`` (needs ``shots``) every shifted circuit is measured on the noisy device, its gate errors, shots and
    readout fields drawn under the circuit's own counter -- csrc/hip/qsim_onchip.hip."""
    _check_shapes(x, w)
    B, n = x.shape
    be = backend if backend not in (None, "auto") else default_backend(x.device)
    mode = resolve_measure("on_chip" if noise is not None else "parameter_shift", shots, noise, trajectories,
                           shift_mask, n, w.shape[-3], be, x.device)
    x = x.detach().float().contiguous()
    w = w.detach().float().contiguous()
    gE = gE.detach().float().contiguous()
    mask = _mask_u8(shift_mask, w)
    ctr0, cptr = split_counter(counter, x.device)
    if be == "cpu":
        return _pshift_rows_cpu(x, w, gE, mask, need_dx, mode.shots or 0, int(seed), ctr0, noise, mode.trajectories)
    G = torch.empty(B, 2 * n * w.shape[-3], device=x.device, dtype=torch.float32)
    if B > 0:
        hip_measured_rows(x, w, gE, G, mode, mask, int(seed), ctr0, cptr, wgroup_of(x, w), need_dx)
    return G


def hip_measured_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, G: torch.Tensor, mode: MeasureMode,
                      mask: Optional[torch.Tensor] = None, seed: int = 0, ctr0: int = 0, counter_ptr=None,
                      wgroup: int = 0, need_dx: bool = True, Ebar: Optional[torch.Tensor] = None) -> None:
    """The per-sample gradient rows G (B, 2nL) fp32 of a mode's own backward: the noise-aware adjoint
    (``Ebar``: nullable, its expectation), else the parameter-shift rule under ``mode.noise`` or without
    (``mask``: nullable, the flat uint8 one).  ``qsim``'s rows functions and the fused step (ops/qsc.py) both launch
    through here."""
    if mode.diff_method == "noisy_adjoint":
        hip_qsim_noisy_adjoint(x, w, gE, G, mode.noise, mode.trajectories, seed, ctr0, counter_ptr, wgroup, Ebar)
    elif mode.noise is not None:
        hip_qsim_noisy_pshift(x, w, gE, G, None, None, mask, need_dx, mode.shots, seed, ctr0, counter_ptr, wgroup,
                              mode.noise, mode.trajectories)
    else:
        hip_qsim_pshift(x, w, gE, G, None, None, mask, need_dx, mode.shots or 0, seed, ctr0, counter_ptr, wgroup)


def _rows_to_grads(G: torch.Tensor, x: torch.Tensor, w: torch.Tensor, be: str, shift_mask=None):
    """(dx, dw) of the gradient rows G (B, 2nL): dx its layer-0 RY columns, dw its sum over the samples."""
    B, n = x.shape
    L = w.shape[-3]
    dx = G[:, 0:2 * n:2].contiguous()
    if be == "hip" and B > 0:   # deterministic: no float atomics
        dw = reduce_slab(G, torch.empty(2 * n * L, device=x.device, dtype=torch.float32))
    else:
        dw = G.sum(0)
    if shift_mask is not None:   # (a masked layer-0 RY column still carries dx)
        dw = dw * _mask_u8(shift_mask, w)
    dw = dw.view(L, n, 2)
    if w.dim() == 4:
        dw = _group_grad(dw, w)
    return dx, dw


class _QSimPShift(torch.autograd.Function):
    """Forward: ``qsim``'s own (exact, finite-shot or noisy).  Backward: parameter shift with the forward's shots,
    seed, counter, noise and trajectories (a device counter is read again by the backward: advance it after the
    backward)."""

    @staticmethod
    def forward(ctx, x, w, be, mode, seed, counter, shift_mask):
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        ctx.save_for_backward(x, w)
        ctx.args = (be, mode, seed, counter, shift_mask)
        return qsim(x, w, be, shots=mode.shots, seed=seed, counter=counter, noise=mode.noise,
                    trajectories=mode.trajectories)

    @staticmethod
    def backward(ctx, gE):
        x, w = ctx.saved_tensors
        be, mode, seed, counter, shift_mask = ctx.args
        G = pshift_rows(x, w, gE, be, mode.shots, seed, counter, shift_mask, need_dx=ctx.needs_input_grad[0],
                        noise=mode.noise, trajectories=mode.trajectories)
        return _rows_to_grads(G, x, w, be, shift_mask) + (None,) * 5


# ----------------------------------------------------------------------------- noise-aware adjoint
def nadj_split(trajectories: int, n: int) -> int:
    """The workgroups per sample csrc/hip/qsim_nadj.hip launches for that many trajectories of n qubits (above 1
    their partial rows are summed in a fixed order: the result is deterministic)."""
    return nat.fn(nat.hip_lib(), "qd_qsim_nadj_split", [_i, _i])(int(trajectories), int(n))


def hip_qsim_noisy_adjoint(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, G: torch.Tensor, noise: "NoiseModel",
                           trajectories: int = 1, seed: int = 0, ctr0: int = 0, counter_ptr=None, wgroup: int = 0,
                           Ebar: Optional[torch.Tensor] = None, frames: Optional[torch.Tensor] = None) -> None:
    """Raw launcher of csrc/hip/qsim_nadj.hip (n <= 12): G (B, 2nL) fp32, the gradient rows of sum(gE * Ebar) with
    Ebar the mean of the noisy shots forward given the Pauli frames it draws under (seed, counter); Ebar (nullable;
    B, n) fp32, frames (nullable; B, T, L, 2) int32 every trajectory's frames."""
    B, n = x.shape
    L = w.shape[-3]
    T = int(trajectories)
    thr1, thr2, thr_ro = noise.thresholds(n, x.device)
    split = nadj_split(T, n) if 2 <= n <= HIP_SHOTS_MAX_QUBITS else 0
    work = torch.empty(split * B * (2 * n * L + n), device=x.device, dtype=torch.float32) if split > 1 else None
    f = nat.fn(nat.hip_lib(), "qd_qsim_noisy_adjoint",
               [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _u64, _u64, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(gE), nat.ptr(G), _opt(Ebar), _opt(frames), _opt(work), nat.ptr(thr1),
                nat.ptr(thr2), nat.ptr(thr_ro), B, n, L, wgroup, T, seed & _M64, ctr0 & _M64, counter_ptr,
                nat.stream_ptr(x.device)), "qd_qsim_noisy_adjoint")


def _nadj_rows_cpu(x, w, gE, noise, T, seed, ctr0):
    """(G, Ebar) composed from the host oracles, in fp64: the frames the noisy forward draws, then the framed
    circuit's exact <Z> of every trajectory -- for Ebar as it stands, for G with one angle shifted by +-pi/2 (the
    shift rule is exact for a circuit with fixed Paulis inserted)."""
    B, n = x.shape
    L = w.shape[-3]
    P = 2 * n * L
    frames = pauli_frames(noise_sites(noise, B, n, L, T, seed, ctr0))
    fr = frames.view(B * T, L, 2)
    xr = x.repeat_interleave(T, dim=0)
    zs = z_signs(n, dtype=torch.float64)
    bits = (frames[:, :, L - 1, 0, None] >> torch.arange(n)) & 1          # (B, T, n): the last X mask
    sgn = (1 - 2 * bits).double()
    thr_ro = torch.from_numpy(noise.thresholds_host(n)[2].astype("int64"))
    c = 1.0 - (thr_ro[:, 0] + thr_ro[:, 1]).double() / 65536.0
    d = (thr_ro[:, 1] - thr_ro[:, 0]).double() / 65536.0

    def mean_z(ws):   # (B, n): mean over the trajectories of s_j E_j
        return ((qsim_probs(xr, ws, "cpu", frames=fr) @ zs).view(B, T, n) * sgn).mean(1)

    Ebar = c * mean_z(w) + d
    gc = gE.double() * c
    G = torch.zeros(B, P, dtype=torch.float64)
    for p in range(P):
        E = []
        for sh in (0.5 * math.pi, -0.5 * math.pi):
            ws = w.clone()
            ws.view(-1, P)[:, p] += sh
            E.append(mean_z(ws))
        G[:, p] = (gc * (E[0] - E[1]) * 0.5).sum(1)
    return G.float(), Ebar


@torch.no_grad()
def noisy_adjoint_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: "NoiseModel", trajectories: int = 1,
                       seed: int = 0, counter=0, backend: Optional[str] = None, return_expectation: bool = False):
    """Per-sample noise-aware adjoint gradients G (B, 2nL) fp32 (``pshift_rows``'s layout: column p = (l n + q) 2 + k
    is w[l, q, k]'s; dx = G[:, 0:2n:2]; dw = G summed over the samples) of sum(gE * Ebar), where, with the Pauli
    frames the noisy forward draws for (``seed``, ``counter``) over ``trajectories`` = T,

        Ebar[b, j] = c_j mean_tau s_j(tau) E_j^tau + d_j

    is the mean of ``qsim(x, w, shots=, noise=, trajectories=T)`` over its outcome and readout draws: E_j^tau the
    exact <Z_j> of trajectory tau's circuit (frames behind the rings of layers 0 .. L-2), s_j(tau) = -1 when the
    last layer's X mask has bit j set, c_j = 1 - (thr01_j + thr10_j) / 65536 and d_j = (thr10_j - thr01_j) / 65536
    from the model's 16-bit readout thresholds.  No shots are needed.  ``return_expectation``: (G, Ebar), Ebar
    (B, n) fp32 on ``hip`` and fp64 on ``cpu`` (as ``qsim_probs``).  csrc/hip/qsim_nadj.hip on ``hip`` (n <= 12), the
    fp64 composition of the host oracles on ``cpu``."""
    _check_shapes(x, w)
    B, n = x.shape
    L = w.shape[-3]
    _check_noise_model(noise)
    T = _check_trajectories(trajectories)
    _check_noise_shape(n, L)
    be = backend if backend not in (None, "auto") else default_backend(x.device)
    x = x.detach().float().contiguous()
    w = w.detach().float().contiguous()
    gE = gE.detach().float().contiguous()
    if tuple(gE.shape) != (B, n):
        raise ValueError(f"gE must be ({B}, {n}), got {tuple(gE.shape)}")
    if be == "torch":
        raise ValueError("the torch backend has no noise model; use hip or cpu")
    _check_backend(be, x.device)
    if be == "hip":
        _hip_shots_limit(n)
        ctr0, cptr = split_counter(counter, x.device)
        G = torch.empty(B, 2 * n * L, device=x.device, dtype=torch.float32)
        Ebar = torch.empty(B, n, device=x.device, dtype=torch.float32) if return_expectation else None
        if B > 0:   # (the rows need no shots: the mode is this function's own)
            hip_measured_rows(x, w, gE, G, MeasureMode("noisy_adjoint", None, noise, T), None, int(seed), ctr0, cptr,
                              wgroup_of(x, w), Ebar=Ebar)
    else:
        _noise_qubit_limit(n)
        ctr0, _ = split_counter(counter, x.device)
        G, Ebar = _nadj_rows_cpu(x, w, gE, noise, T, int(seed), ctr0)
    return (G, Ebar) if return_expectation else G


class _QSimNoisyAdjoint(torch.autograd.Function):
    """Forward: the noisy finite-shot forward, unchanged.  Backward: the adjoint through the Pauli frames that
    forward sampled -- the same seed, counter and trajectories (a device counter is read again by the backward:
    advance it after the backward)."""

    @staticmethod
    def forward(ctx, x, w, be, mode, seed, counter):
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        ctx.save_for_backward(x, w)
        ctx.args = (be, mode, seed, counter)
        return _measured_fwd(x, w, be, mode, seed, *split_counter(counter, x.device))

    @staticmethod
    def backward(ctx, gE):
        x, w = ctx.saved_tensors
        be, mode, seed, counter = ctx.args
        G = noisy_adjoint_rows(x, w, gE, mode.noise, mode.trajectories, seed, counter, be)
        return _rows_to_grads(G, x, w, be) + (None,) * 4


def _check_hip_adjoint(n: int, L: int) -> None:
    """What the exact HIP simulators run: the forward of the exact mode, the backward of the straight-through ones."""
    if n > HIP_MAX_QUBITS:
        raise NotImplementedError(f"HIP simulators support n <= {HIP_MAX_QUBITS}")
    if 2 * n * L > 256 and n > HIP_REG_MAX_QUBITS:
        raise NotImplementedError("large-n HIP simulator supports 2*n*L <= 256")


def qsim(x: torch.Tensor, w: torch.Tensor, backend: Optional[str] = None, shots: Optional[int] = None, seed: int = 0,
         counter=0, diff_method: str = "adjoint", shift_mask: Optional[torch.Tensor] = None,
         noise: Optional["NoiseModel"] = None, trajectories: int = 1) -> torch.Tensor:
    """<Z_i> of the QSC circuit for inputs x (B, n) and weights w (L, n, 2).

    ``w`` may also be grouped, (G, L, n, 2) with B % G == 0: sample b then uses
    w[b // (B/G)] (independent QuantumNAT noise per data stream).

    ``shots`` (None / 0: the exact expectation): every <Z_i> is estimated from that many measurement shots of
    the final state -- the fused kernel of csrc/hip/qsim_shots.hip on ``hip`` (n <= 12; n = 13..16 with L >= 2 on
    the streamed simulator, csrc/hip/qsim_stream_shots.hip, without noise and with the adjoint gradient only),
    simulate-then-sample
    on ``cpu``; ``torch`` has no sampler.  The shots of a call are a function of (``seed``, ``counter``, row);
    ``counter`` is an int, or on ``hip`` a CUDA int64 / uint64 scalar tensor the kernel reads (advance it with
    ``counter_add`` after the call: graph replays then draw fresh shots).  The BACKWARD is the exact adjoint of
    the same (x, w): shot noise is straight-through, the way QuantumNAT's weight noise is treated.

    ``diff_method="parameter_shift"`` (``hip`` with n <= 12, or ``cpu``) keeps that forward and replaces the
    backward by the parameter-shift rule: every gradient entry comes from two more runs of the circuit with one
    angle shifted by +-pi/2, each measured with the forward's ``shots`` (None: exactly) -- csrc/hip/qsim_pshift.hip.
    Shifted circuit (p, s) draws under counter + ((1 + 2p + s) << 48), so its shots never coincide with the
    forward's or another circuit's for counters below 2^48.  ``shift_mask`` ((L, n, 2) bool, None: all): the
    parameters whose circuits run; the others get a gradient of exactly 0 (``x``'s gradient is unaffected).

    ``noise`` (a ``NoiseModel``; needs ``shots``; ``hip`` with n <= 12, or ``cpu``): the shots are measured on a
    device with Pauli gate errors and readout error -- csrc/hip/qsim_noise.hip.  The shots are split evenly over
    ``trajectories`` (1 .. 1024) independent realisations of the gate errors; trajectory t owns shots
    [t shots/T, (t+1) shots/T), and for T > 1 shots / T must be a multiple of 4.  With all rates zero the result is
    bit-identical to the noiseless ``shots`` call.  The backward stays the exact adjoint of the noiseless circuit
    (straight-through); ``diff_method="parameter_shift"`` is not available under noise.

    ``diff_method="on_chip"`` (needs ``shots``; ``hip`` with n <= 12, or ``cpu``): the gradient a device reports.
    The forward is the call's own (noisy shots with ``noise``, else plain shots); the backward is the
    parameter-shift rule with every shifted circuit measured with the same ``shots``, ``noise`` and
    ``trajectories``, its error sites, shots and readout fields drawn under its own counter
    counter + ((1 + 2p + s) << 48) -- csrc/hip/qsim_onchip.hip.  ``shift_mask`` is allowed; with ``noise=None`` it
    is ``"parameter_shift"`` bit for bit.

    ``diff_method="noisy_adjoint"`` (needs ``noise`` and ``shots``; ``hip`` with n <= 12, or ``cpu``): training
    against the device model on a simulator.  The forward is the noisy shots call unchanged; the backward
    differentiates through the circuit with the sampled error gates in it -- the adjoint method run through the
    Pauli frames the forward drew under the same ``seed`` / ``counter`` / ``trajectories``, weighted by the last
    frame's outcome flips and the readout thresholds (``noisy_adjoint_rows``; csrc/hip/qsim_nadj.hip).  It is the
    exact gradient of the forward's mean given those frames, at roughly (1 + rebuilding trajectories) adjoint
    passes per sample.  A device ``counter`` is read again by the backward: advance it after the backward.
    ``shift_mask`` is not available."""
    _check_shapes(x, w)
    n, L = x.shape[1], w.shape[-3]
    be = backend if backend not in (None, "auto") else default_backend(x.device)
    mode = resolve_measure(diff_method, shots, noise, trajectories, shift_mask, n, L, be, x.device)
    if mode.diff_method == "noisy_adjoint":
        return _QSimNoisyAdjoint.apply(x, w, be, mode, int(seed), counter)
    if mode.diff_method != "adjoint":   # the parameter-shift family
        return _QSimPShift.apply(x, w, be, mode, int(seed), counter, shift_mask)
    if mode.shots and be == "hip":   # straight-through: the measured forward, the exact adjoint's backward
        _check_hip_adjoint(n, L)
        return _QSimMeasuredHIP.apply(x, w, mode, int(seed), *split_counter(counter, x.device))
    if mode.shots:   # the exact forward for the graph, its values replaced by the measured ones
        ctr0, _ = split_counter(counter, x.device)
        E = _measured_fwd(x.detach().float().contiguous(), w.detach().float().contiguous(), be, mode, int(seed), ctr0)
        return _ReplaceValue.apply(qsim(x, w, "cpu"), E)
    _check_backend(be, x.device)
    if be == "hip":
        _check_hip_adjoint(n, L)
        return _QSimHIP.apply(x, w, wgroup_of(x, w))
    if w.dim() == 4:  # host backends: run per group
        return torch.cat([qsim(xc, w[g], be) for g, xc in enumerate(x.chunk(w.shape[0]))], dim=0)
    return _QSimCPU.apply(x, w) if be == "cpu" else qsim_torch(x, w)


# ----------------------------------------------------------------------------- exact noisy expectation
MIXED_MAX_QUBITS = 8             # csrc/hip/qsim_mixed.hip: rho in LDS to 7 qubits, in a workspace slot at 8
MIXED_ROWS_BYTES = 32 << 20      # mixed_rows: the shifted circuits' extra rows (x, w, E) of one chunk of parameters


def _mixed_backend(x: torch.Tensor, w: torch.Tensor, noise, backend: Optional[str]) -> str:
    """The refusals of the density-matrix functions, before any launch; returns the backend."""
    _check_shapes(x, w)
    if not isinstance(noise, NoiseModel):
        raise ValueError(f"the density-matrix simulator needs noise=NoiseModel(...) (all-zero rates are allowed), got "
                         f"{type(noise).__name__}")
    n, L = x.shape[1], w.shape[-3]
    be = backend if backend not in (None, "auto") else default_backend(x.device)
    if be == "torch":
        raise ValueError("the torch backend has no density-matrix simulator; use hip or cpu")
    if be not in ("hip", "cpu"):
        raise ValueError(f"unknown backend {be!r}")
    if n > MIXED_MAX_QUBITS:   # (the host oracle keeps the kernel's range: one contract)
        raise NotImplementedError(f"the density-matrix simulator supports n <= {MIXED_MAX_QUBITS} qubits "
                                  f"(rho has 4^n entries), got {n}")
    if 2 * n * L > MAX_NOISE_SITES:
        raise ValueError(f"the density-matrix simulator supports 2 n L <= {MAX_NOISE_SITES} error sites, got n={n} L={L}")
    want = "cuda" if be == "hip" else "cpu"
    if x.device.type != want or w.device.type != want:
        raise ValueError(f"the {be} density-matrix simulator needs {want.upper()} tensors, got x on {x.device} and w on "
                         f"{w.device}")
    return be


def mixed_force_grid(grid: int) -> None:
    """Tests and timing: csrc/hip/qsim_mixed.hip launches at most ``grid`` workgroups from now on; 0 hands the choice
    back to the launcher."""
    nat.check(nat.fn(nat.hip_lib(), "qd_qsim_mixed_force_grid", [_i])(int(grid)), "qd_qsim_mixed_force_grid")


def hip_qsim_mixed_fwd(x: torch.Tensor, w: torch.Tensor, E: torch.Tensor, probs: Optional[torch.Tensor],
                       noise: NoiseModel, wgroup: int = 0, ws: Optional[torch.Tensor] = None) -> None:
    """Raw launcher of csrc/hip/qsim_mixed.hip (2 <= n <= 8): E (B, n) fp32, the exact expectation of the device
    under ``noise``; probs (nullable; B, 2^n) fp32, the diagonal of rho before the readout.  ``ws``: a workspace of at
    least qd_qsim_mixed_workspace(n, B) bytes to use instead of allocating one (n = 8)."""
    lib = nat.hip_lib()
    B, n = x.shape
    thr1, thr2, thr_ro = noise.thresholds(n, x.device)
    nbytes = nat.fn(lib, "qd_qsim_mixed_workspace", [_i, _i], ctypes.c_longlong)(n, B)
    if ws is not None and ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"the workspace holds {ws.numel() * ws.element_size()} bytes, the launch needs {nbytes}")
    if ws is None and nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    f = nat.fn(lib, "qd_qsim_mixed_fwd", [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(thr1), nat.ptr(thr2), nat.ptr(thr_ro), nat.ptr(E), _opt(probs), B, n,
                w.shape[-3], wgroup, _opt(ws), nat.stream_ptr(x.device)), "qd_qsim_mixed_fwd")


def mixed_readout(noise: NoiseModel, n: int):
    """(c, d) (n) fp64 of the readout's affine map E_i = c_i <Z_i> + d_i: c_i = 1 - (thr01_i + thr10_i) / 65536,
    d_i = (thr10_i - thr01_i) / 65536 from the model's 16-bit thresholds (as ``noisy_adjoint_rows``)."""
    thr_ro = torch.from_numpy(noise.thresholds_host(n)[2].astype("int64"))
    return (1.0 - (thr_ro[:, 0] + thr_ro[:, 1]).double() / 65536.0,
            (thr_ro[:, 1] - thr_ro[:, 0]).double() / 65536.0)


def _mixed_probs_cpu(x: torch.Tensor, w: torch.Tensor, noise: NoiseModel) -> torch.Tensor:
    B, n = x.shape
    if w.dim() == 4:   # the host oracle runs per group
        return torch.cat([_mixed_probs_cpu(xc, w[g], noise) for g, xc in enumerate(x.chunk(w.shape[0]))], dim=0)
    thr1, thr2, _ = noise.thresholds(n, "cpu")
    probs = torch.empty(B, 1 << n, dtype=torch.float64)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_qsim_mixed_probs", [_p, _p, _p, _p, _p, _i, _i, _i])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(thr1), nat.ptr(thr2), nat.ptr(probs), B, n, w.shape[0]),
              "qd_cpu_qsim_mixed_probs")
    return probs


@torch.no_grad()
def _mixed_fwd(x: torch.Tensor, w: torch.Tensor, noise: NoiseModel, be: str, want_probs: bool = False):
    """E (B, n), or the probabilities (B, 2^n): fp32 on ``hip``, fp64 on ``cpu``; x, w checked, fp32, contiguous."""
    B, n = x.shape
    if be == "hip":
        E = torch.empty(B, n, device=x.device, dtype=torch.float32)
        probs = torch.empty(B, 1 << n, device=x.device, dtype=torch.float32) if want_probs else None
        if B > 0:
            hip_qsim_mixed_fwd(x, w, E, probs, noise, wgroup_of(x, w))
        return probs if want_probs else E
    probs = _mixed_probs_cpu(x, w, noise)
    if want_probs:
        return probs
    c, d = mixed_readout(noise, n)
    return c * (probs @ z_signs(n, dtype=torch.float64)) + d


def qsim_mixed_probs(x: torch.Tensor, w: torch.Tensor, noise: NoiseModel, backend: Optional[str] = None) -> torch.Tensor:
    """Outcome probabilities (B, 2^n) of the noisy device before the readout error, natural basis order: the diagonal
    of the density matrix ``qsim_mixed`` evolves.  fp32 on ``hip``, fp64 on ``cpu``.  No autograd."""
    be = _mixed_backend(x, w, noise, backend)
    return _mixed_fwd(x.detach().float().contiguous(), w.detach().float().contiguous(), noise, be, want_probs=True)


def _mixed_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: NoiseModel, be: str) -> torch.Tensor:
    B, n = x.shape
    L = w.shape[-3]
    P = 2 * n * L
    wg = w.reshape(-1, P)                       # (G0, P): the call's own weight groups
    G0 = wg.shape[0]
    per = 2 * (B * 2 * n + G0 * P) * 4          # bytes of one parameter's two circuits: x and E rows, weights
    step = max(1, min(P, MIXED_ROWS_BYTES // per))
    g = gE.double() if be == "cpu" else gE      # (E carries the readout's c; its d cancels in the difference)
    G = torch.empty(B, P, device=x.device, dtype=torch.float32)
    shift = torch.tensor([0.5 * math.pi, -0.5 * math.pi], device=x.device)
    for p0 in range(0, P, step):
        k = min(step, P - p0)
        ws = wg.repeat(k, 2, 1, 1)              # (k, 2, G0, P): parameter p0 + i shifted by +-pi/2
        idx = torch.arange(k, device=x.device)
        ws[idx, :, :, p0 + idx] += shift[None, :, None]
        E = _mixed_fwd(x.repeat(2 * k, 1), ws.view(2 * k * G0, L, n, 2), noise, be).view(k, 2, B, n)
        G[:, p0:p0 + k] = ((E[:, 0] - E[:, 1]) * g).sum(-1).mul_(0.5).t()
    return G


@torch.no_grad()
def mixed_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: NoiseModel, backend: Optional[str] = None,
               need_dx: bool = True) -> torch.Tensor:
    """Per-sample gradients G (B, 2nL) fp32 of sum(gE * qsim_mixed(x, w, noise)), in ``pshift_rows``'s layout: column
    p = (l n + q) 2 + k is w[l, q, k]'s; dx = G[:, 0:2n:2]; dw = G summed over the samples.  The +-pi/2 shift rule,
    exact here (the channel is linear and every generator has two eigenvalues): two forward evaluations per parameter,
    launched over the shifted weights as grouped ``w``, in chunks of parameters whose extra rows stay under
    ``MIXED_ROWS_BYTES``.  ``need_dx`` is accepted for symmetry with ``pshift_rows``: every column is computed."""
    be = _mixed_backend(x, w, noise, backend)
    B, n = x.shape
    if tuple(gE.shape) != (B, n):
        raise ValueError(f"gE must be ({B}, {n}), got {tuple(gE.shape)}")
    if gE.device != x.device:
        raise ValueError(f"gE must be on {x.device}, got {gE.device}")
    return _mixed_rows(x.detach().float().contiguous(), w.detach().float().contiguous(),
                       gE.detach().float().contiguous(), noise, be)


MIXED_DIFF_METHODS = ("parameter_shift", "adjoint")
MIXED_ADJOINT_MAX_THR = 1 << 31   # p <= 1/2: the adjoint inverts the sites, and 1 / (1 - 4p/3) grows without bound


def _check_adjoint_rates(noise: NoiseModel, n: int) -> None:
    """The adjoint's limit, on the integer thresholds the kernels use."""
    thr1, thr2, _ = noise.thresholds_host(n)
    if int(thr1.max()) > MIXED_ADJOINT_MAX_THR or int(thr2.max()) > MIXED_ADJOINT_MAX_THR:
        raise ValueError("the density-matrix adjoint undoes every error site and needs p1, p2 <= 0.5 on every wire "
                         f"(got p1 up to {float(thr1.max()) / 2 ** 32:.4f}, p2 up to {float(thr2.max()) / 2 ** 32:.4f});"
                         ' use diff_method="parameter_shift"')


def mixed_adjoint_workspace(n: int, B: int, device) -> Optional[torch.Tensor]:
    """The workspace of ``hip_qsim_mixed_adjoint`` for a batch of B (n = 7, 8: rho and Lambda of every workgroup), or
    None where it needs none."""
    nbytes = nat.fn(nat.hip_lib(), "qd_qsim_mixed_adjoint_workspace", [_i, _i], ctypes.c_longlong)(n, B)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def hip_qsim_mixed_adjoint(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, G: torch.Tensor,
                           E: Optional[torch.Tensor], noise: NoiseModel, wgroup: int = 0,
                           ws: Optional[torch.Tensor] = None) -> None:
    """Raw launcher of csrc/hip/qsim_mixed.hip's adjoint (2 <= n <= 8, rates <= 0.5): G (B, 2nL) fp32, the gradient
    rows of sum(gE * E) in ``pshift_rows``'s layout, in one launch; E (nullable; B, n) ``hip_qsim_mixed_fwd``'s, bit
    for bit.  ``ws``: ``mixed_adjoint_workspace(n, B, device)``, allocated here when not given."""
    B, n = x.shape
    _check_adjoint_rates(noise, n)
    thr1, thr2, thr_ro = noise.thresholds(n, x.device)
    if ws is None:
        ws = mixed_adjoint_workspace(n, B, x.device)
    else:
        need = nat.fn(nat.hip_lib(), "qd_qsim_mixed_adjoint_workspace", [_i, _i], ctypes.c_longlong)(n, B)
        if ws.numel() * ws.element_size() < need:
            raise ValueError(f"the workspace holds {ws.numel() * ws.element_size()} bytes, the launch needs {need}")
    f = nat.fn(nat.hip_lib(), "qd_qsim_mixed_adjoint", [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(thr1), nat.ptr(thr2), nat.ptr(thr_ro), nat.ptr(gE), nat.ptr(G), _opt(E),
                B, n, w.shape[-3], wgroup, _opt(ws), nat.stream_ptr(x.device)), "qd_qsim_mixed_adjoint")


def _mixed_adjoint_cpu(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: NoiseModel) -> torch.Tensor:
    """G (B, 2nL) fp64 of the complex128 host twin (csrc/cpu/qsim_cpu.cpp qd_cpu_qsim_mixed_adjoint)."""
    B, n = x.shape
    if w.dim() == 4:   # the host twin runs per group
        return torch.cat([_mixed_adjoint_cpu(xc, w[g], gc, noise)
                          for g, (xc, gc) in enumerate(zip(x.chunk(w.shape[0]), gE.chunk(w.shape[0])))], dim=0)
    thr1, thr2, thr_ro = noise.thresholds(n, "cpu")
    G = torch.empty(B, 2 * n * w.shape[0], dtype=torch.float64)
    f = nat.fn(nat.cpu_lib(), "qd_cpu_qsim_mixed_adjoint", [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i])
    nat.check(f(nat.ptr(x), nat.ptr(w), nat.ptr(thr1), nat.ptr(thr2), nat.ptr(thr_ro), nat.ptr(gE), nat.ptr(G), None,
                B, n, w.shape[0]), "qd_cpu_qsim_mixed_adjoint")
    return G


def _mixed_adjoint_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: NoiseModel, be: str) -> torch.Tensor:
    B, n = x.shape
    if be == "cpu":
        return _mixed_adjoint_cpu(x, w.contiguous(), gE, noise).float()
    G = torch.empty(B, 2 * n * w.shape[-3], device=x.device, dtype=torch.float32)
    if B > 0:
        hip_qsim_mixed_adjoint(x, w, gE, G, None, noise, wgroup_of(x, w))
    return G


@torch.no_grad()
def mixed_adjoint_rows(x: torch.Tensor, w: torch.Tensor, gE: torch.Tensor, noise: NoiseModel,
                       backend: Optional[str] = None) -> torch.Tensor:
    """``mixed_rows``'s G (B, 2nL) fp32 by reverse-mode differentiation of the channel: the forward recomputed, then
    rho and the observable carried back through the sweeps, every error site undone on rho (csrc/hip/qsim_mixed.hip
    qd_qsim_mixed_adjoint in one launch on ``hip``, its complex128 twin on ``cpu``) -- a few forward-equivalents
    instead of 4 n L.  Undoing a site divides by 1 - 4 p1 / 3 (1 - 16 p2 / 15), so every rate must be <= 0.5; the other
    refusals are ``mixed_rows``'s."""
    be = _mixed_backend(x, w, noise, backend)
    B, n = x.shape
    if tuple(gE.shape) != (B, n):
        raise ValueError(f"gE must be ({B}, {n}), got {tuple(gE.shape)}")
    if gE.device != x.device:
        raise ValueError(f"gE must be on {x.device}, got {gE.device}")
    _check_adjoint_rates(noise, n)
    return _mixed_adjoint_rows(x.detach().float().contiguous(), w.detach().float().contiguous(),
                               gE.detach().float().contiguous(), noise, be)


class _QSimMixed(torch.autograd.Function):
    """Forward: the exact noisy expectation.  Backward: its exact gradient, ``mixed_rows`` or (``adjoint``)
    ``mixed_adjoint_rows``."""

    @staticmethod
    def forward(ctx, x, w, noise, be, adjoint=False):
        x = x.detach().float().contiguous()
        w = w.detach().float().contiguous()
        ctx.save_for_backward(x, w)
        ctx.args = (noise, be, adjoint)
        return _mixed_fwd(x, w, noise, be).float()

    @staticmethod
    def backward(ctx, gE):
        x, w = ctx.saved_tensors
        noise, be, adjoint = ctx.args
        rows = _mixed_adjoint_rows if adjoint else _mixed_rows
        G = rows(x, w, gE.detach().float().contiguous(), noise, be)
        return _rows_to_grads(G, x, w, be) + (None, None, None)


def qsim_mixed(x: torch.Tensor, w: torch.Tensor, noise: NoiseModel, backend: Optional[str] = None,
               diff_method: str = "parameter_shift") -> torch.Tensor:
    """<Z_i> (B, n) fp32 of the QSC circuit on the noisy device itself: the expectation that
    ``qsim(x, w, shots=, noise=, trajectories=)`` estimates, with no Monte-Carlo error -- the density matrix evolved
    through the circuit with, in expectation, the Pauli channel the sampling kernels draw from (after wire q's fused
    RZ.RY a uniformly drawn X / Y / Z with probability thr1[q] / 2^32, after every CNOT with control q a uniformly
    drawn non-identity two-qubit Pauli with probability thr2[q] / 2^32), then the readout's affine map
    (``mixed_readout``).  The rates are the model's integer thresholds, so a sampler's mean converges to exactly this.

    2 <= n <= 8 (rho has 4^n entries) and 2 n L <= 4096 on both backends: csrc/hip/qsim_mixed.hip on ``hip``, the
    complex128 gate-by-gate oracle of csrc/cpu/qsim_cpu.cpp on ``cpu``; ``torch`` has none.  ``w`` may be grouped as
    for ``qsim``.  An all-zero ``NoiseModel`` gives the noiseless expectation.  Differentiable in x and w: by default
    the backward is ``mixed_rows`` (two forward evaluations per parameter); ``diff_method="adjoint"`` makes it
    ``mixed_adjoint_rows`` (one launch; every gate rate <= 0.5)."""
    be = _mixed_backend(x, w, noise, backend)
    if diff_method not in MIXED_DIFF_METHODS:
        raise ValueError(f"qsim_mixed: diff_method must be one of {MIXED_DIFF_METHODS}, got {diff_method!r}")
    if diff_method == "adjoint":
        _check_adjoint_rates(noise, x.shape[1])
    return _QSimMixed.apply(x, w, noise, be, diff_method == "adjoint")


def init_weights_(w: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """PennyLane TorchLayer default init: U[0, 2*pi)."""
    with torch.no_grad():
        w.uniform_(0.0, 2 * math.pi, generator=generator)
    return w
