"""Estimator / classifier modules with the reference's class names and state_dict keys.

Reference: Estimators_QuantumNAT_onchipQNN.py
  DCE_P128  E:40-75     flat deep channel estimator (Conv stack + FC in one module)
  SC_P128   E:79-101    classical scenario classifier
  QSC_P128  E:107-228   hybrid CNN -> VQC -> linear scenario classifier
  Conv_P128 E:237-268   per-scenario feature extractor
  FC_P128   E:272-279   shared feature mapper 4096 -> 2048
  NMSE_cuda / NMSELoss  E:282-295

Layer indices inside ``nn.Sequential`` containers, parameter names and registration
order are kept identical so checkpoints load in both directions (SURVEY.md §2.1
"Checkpoint keys").  The compute behind them is MI355X-native: the quantum layer runs
on the HIP state-vector kernels (ops/quantum.py), the classical layers through the
fused kernels in ops/ when driven by the training engines (train/engine.py).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.quantum import qsim, qsim_mixed, init_weights_

PILOT_GRID = {128: (16, 8), 256: (16, 16)}  # P128 is the reference grid (R:108); P256 is ours


def pilot_grid(pilot_num: int):
    if pilot_num not in PILOT_GRID:
        raise ValueError(f"unsupported Pilot_num {pilot_num}; known: {sorted(PILOT_GRID)}")
    return PILOT_GRID[pilot_num]


def _cnn_stack(features: int = 32, kernel_size: int = 3, padding: int = 1) -> nn.Sequential:
    layers = [nn.Conv2d(2, features, kernel_size, stride=1, padding=padding, bias=False),
              nn.BatchNorm2d(features), nn.ReLU(inplace=True)]
    for _ in range(2):
        layers += [nn.Conv2d(features, features, kernel_size, stride=1, padding=padding, bias=False),
                   nn.BatchNorm2d(features), nn.ReLU(inplace=True)]
    return nn.Sequential(*layers)


class DCE_P128(nn.Module):
    """Flat estimator: 3x[conv3x3 -> BN -> ReLU] then Linear(32*H*W, 2048) (E:40-75)."""

    def __init__(self, pilot_num: int = 128, out_dim: int = 64 * 16 * 2):
        super().__init__()
        self.features, self.kernel_size, self.padding = 32, 3, 1
        self.H, self.W = pilot_grid(pilot_num)
        self.cnn = _cnn_stack(self.features, self.kernel_size, self.padding)
        self.FC = nn.Linear(self.features * self.H * self.W, out_dim)

    def forward(self, x):
        x = self.cnn(x)
        return self.FC(x.reshape(x.shape[0], self.features * self.H * self.W))


class SC_P128(nn.Module):
    """Classical scenario classifier (E:79-101): conv-relu-pool x2 -> Linear -> log_softmax."""

    def __init__(self, pilot_num: int = 128, n_classes: int = 3):
        super().__init__()
        H, W = pilot_grid(pilot_num)
        self.pilot_num = pilot_num
        self.flat = 32 * (H // 4) * (W // 4)
        self.conv1 = nn.Conv2d(2, 32, kernel_size=3, padding=1, bias=False)
        self.conv2 = nn.Conv2d(32, 32, kernel_size=3, padding=1, bias=False)
        self.FC = nn.Linear(self.flat, n_classes)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.conv1(x)), 2, 2)
        x = F.max_pool2d(F.relu(self.conv2(x)), 2, 2)
        return F.log_softmax(self.FC(x.reshape(x.shape[0], self.flat)), dim=1)


class QuantumLayer(nn.Module):
    """Drop-in for PennyLane's ``qml.qnn.TorchLayer`` (E:144-149): owns ``weights``
    of shape (n_layers, n_qubits, 2), maps (B, n) angles to (B, n) <Z_i> values.

    ``shots`` (settable; None / 0 = exact expectations) is the device's ``shots=``: every <Z_i> is then
    estimated from that many measurement shots (ops/quantum.py ``qsim(shots=)``; by default gradients stay
    exact, straight-through).  The shot stream is keyed by ``shot_seed`` and a Python-side call counter that
    every forward advances, so successive calls draw different shots; ``manual_shot_seed`` restarts it.
    Neither is a parameter or a buffer: the state_dict is that of the exact layer.

    ``diff_method`` (settable; "adjoint", "parameter_shift" or "on_chip") selects the backward: the exact adjoint,
    the parameter-shift rule measured with the same ``shots``, or with "on_chip" (needs ``shots``) that rule measured
    under the same ``noise`` and ``trajectories`` as well (``qsim(diff_method=)``).  ``shift_mask`` (settable;
    None or a (n_layers, n_qubits, 2) bool tensor) names the parameters whose shifted circuits run; the others
    get a zero gradient.  Both are plain attributes too.

    ``noise`` (settable; None or an ``ops.quantum.NoiseModel``) and ``trajectories`` (settable; 1 .. 1024) measure
    the shots on a device with Pauli gate errors and readout error (``qsim(noise=, trajectories=)``); they need
    ``shots``, and gradients stay those of the noiseless circuit unless ``diff_method`` is "on_chip" or
    "noisy_adjoint" (needs ``noise`` and ``shots``: the adjoint through the error gates the forward sampled).

    ``exact_noise`` (settable; default False): with ``noise`` set and ``shots`` not, the forward is the exact
    expectation of the noisy device, ``ops.quantum.qsim_mixed`` (n <= 8; its gradient is the exact one), instead of
    the refusal "noise needs shots".  ``exact_diff_method`` (settable; "parameter_shift" by default, or "adjoint")
    is that forward's backward (``qsim_mixed(diff_method=)``): the shift rule over forward launches, or the one-launch
    adjoint through the channel (gate rates <= 0.5)."""

    def __init__(self, n_qubits: int, n_layers: int, backend: Optional[str] = None, shots: Optional[int] = None,
                 diff_method: str = "adjoint", noise=None, trajectories: int = 1):
        super().__init__()
        self.n_qubits, self.n_layers = n_qubits, n_layers
        self.backend = backend
        self.shots = shots
        self.diff_method = diff_method
        self.shift_mask = None
        self.noise = noise
        self.trajectories = trajectories
        self.exact_noise = False   # True (with noise and no shots): the exact expectation of the noisy device
        self.exact_diff_method = "parameter_shift"   # ... and its backward: the shift rule, or "adjoint" (one launch)
        self.shot_seed = 0
        self._shot_calls = 0
        self.keep_input = False   # True: every forward leaves its angles, detached, in last_input (ops/qng.py reads them)
        self.last_input = None
        self.weights = nn.Parameter(init_weights_(torch.empty(n_layers, n_qubits, 2)))

    def manual_shot_seed(self, seed: int) -> None:
        """Seed the shot stream and restart its call counter."""
        self.shot_seed = int(seed)
        self._shot_calls = 0

    def forward(self, x: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        w = self.weights if weights is None else weights
        if self.keep_input:
            self.last_input = x.detach()
        if self.exact_noise and self.noise is not None and not self.shots:
            # the default makes the four-argument call it always made: tests/test_mixed_cpu.py replaces qsim_mixed
            # with a function of exactly those arguments
            if self.exact_diff_method == "parameter_shift":
                return qsim_mixed(x.float(), w, self.noise, self.backend)
            return qsim_mixed(x.float(), w, self.noise, self.backend, diff_method=self.exact_diff_method)
        kw = {} if self.diff_method == "adjoint" else {"diff_method": self.diff_method, "shift_mask": self.shift_mask}
        if self.noise is not None:
            kw.update(noise=self.noise, trajectories=int(self.trajectories))
        if not self.shots:
            return qsim(x.float(), w, self.backend, **kw)
        call = self._shot_calls
        self._shot_calls += 1
        return qsim(x.float(), w, self.backend, shots=int(self.shots), seed=self.shot_seed, counter=call, **kw)

    def extra_repr(self) -> str:
        return (f"n_qubits={self.n_qubits}, n_layers={self.n_layers}, backend={self.backend}, shots={self.shots}, "
                f"shot_seed={self.shot_seed}, diff_method={self.diff_method}")


class PostMeasurement(nn.Module):
    """QuantumNAT post-measurement normalization and (``levels`` >= 2) quantization of the measured <Z_j> (B, n):
    ``ops.postmeas.post_measurement`` with ``BatchNorm1d(n, affine=False)``'s running statistics as buffers.

    Training normalizes with the batch's statistics and updates the running ones; evaluation uses the batch's own
    statistics (``stats="batch"``, the default: a noisy device's affine distortion of <Z_j> is removed without
    knowing it, but a prediction depends on the batch it is in) or the running ones (``stats="running"``).
    ``forward(E, valid=None)`` returns the head's input and leaves the normalized values (detached) in ``self.z`` and
    ``weight * sum (z - Q)^2 / (valid * n)`` in ``self.penalty`` (a 0-d tensor the loss adds)."""

    def __init__(self, n: int, levels: int = 0, qrange: float = 2.0, weight: float = 0.0, momentum: float = 0.1,
                 eps: float = 1e-5, stats: str = "batch"):
        super().__init__()
        from ..ops.postmeas import STATS, check_quantizer
        check_quantizer(int(levels), float(qrange), float(weight))
        if stats not in STATS:
            raise ValueError(f"unknown post-measurement stats {stats!r}: one of {STATS}")
        self.n, self.levels, self.qrange, self.weight = int(n), int(levels), float(qrange), float(weight)
        self.momentum, self.eps, self.stats = float(momentum), float(eps), stats
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self.penalty = None   # set by every forward, on the input's device
        self.z = None

    def forward(self, E: torch.Tensor, valid: Optional[int] = None) -> torch.Tensor:
        from ..ops.postmeas import post_measurement
        y, z, pen = post_measurement(E, self.running_mean, self.running_var, training=self.training,
                                     stats=self.stats, momentum=self.momentum, eps=self.eps, levels=self.levels,
                                     qrange=self.qrange, valid=valid)
        rows = E.shape[0] if valid is None else int(valid)
        self.z = z.detach()
        self.penalty = pen * (self.weight / (rows * self.n))
        return y

    def extra_repr(self) -> str:
        return (f"n={self.n}, levels={self.levels}, qrange={self.qrange}, weight={self.weight}, "
                f"momentum={self.momentum}, eps={self.eps}, stats={self.stats}")


class QSC_P128(nn.Module):
    """Quantum scenario classifier (E:107-228).

    preprocess CNN -> tanh angles -> VQC (<Z_i>) -> Linear(n, n_classes) -> log_softmax.

    QuantumNAT (E:175-199): the reference perturbs the qlayer parameters in place,
    runs the forward, and restores them *before* backward, so autograd mixes noisy
    intermediates with clean leaves.  Here the semantics are explicit: forward AND
    backward use w + noise_level*N(0,1); the gradient is applied to the clean master
    weights (straight-through), and the master weights are never mutated.
    On-chip gradient pruning (E:205-228) zeroes every gradient with |g| <= threshold
    for ALL parameters (classical included), as the reference does.
    ``use_quantum=False`` selects ``classical_fallback`` (referenced at E:168-170 but never
    defined there): Linear(n, n) + Tanh in place of the VQC, an equal-width classical ablation
    with the same (-1, 1) output range as <Z_i>.
    ``shots`` goes to the ``qlayer`` (finite-shot <Z_i>; None = exact), and so does ``diff_method``
    ("adjoint", "parameter_shift": the gradient an on-chip QNN measures, "on_chip": that gradient measured
    under ``noise`` too, or "noisy_adjoint": the exact gradient through the sampled error gates), ``noise`` and ``trajectories`` (the device's gate and readout errors under which the
    shots are measured).
    ``post_norm`` adds QuantumNAT's post-measurement normalization between the measurement and the head
    (``self.postmeas``, a ``PostMeasurement``; registered last, so the default model's state_dict is untouched), and
    ``post_quant_levels`` >= 2 its post-measurement quantization to that many levels on +-``post_quant_range`` with
    the quadratic penalty weighted by ``post_quant_weight``.  Both are off by default.
    """

    def __init__(self, n_qubits: int = 6, n_layers: int = 3, n_classes: int = 3, use_quantumnat: bool = True,
                 use_gradient_pruning: bool = True, pilot_num: int = 128, backend: Optional[str] = None,
                 noise_level: float = 0.01, gradient_threshold: float = 0.1, use_quantum: bool = True,
                 shots: Optional[int] = None, diff_method: str = "adjoint", noise=None, trajectories: int = 1,
                 post_norm: bool = False, post_quant_levels: int = 0, post_quant_range: float = 2.0,
                 post_quant_weight: float = 0.0):
        super().__init__()
        from ..ops.postmeas import check_quantizer
        check_quantizer(int(post_quant_levels), float(post_quant_range), float(post_quant_weight))
        if post_quant_levels and not post_norm:
            raise ValueError("post_quant_levels needs post_norm: the quantizer's levels sit on the normalized scale")
        self.use_quantum = use_quantum
        self.num_qubits = n_qubits
        self.n_layers = n_layers
        self.n_classes = n_classes
        self.use_quantumnat = use_quantumnat
        self.use_gradient_pruning = use_gradient_pruning
        self.noise_level = noise_level if use_quantumnat else 0.0
        self.gradient_threshold = gradient_threshold
        self.last_pruning_ratio = 0.0
        H, W = pilot_grid(pilot_num)
        flat = 32 * (H // 4) * (W // 4)
        # registration order matters: qlayer.weights is the first state_dict key (E:149 < E:152)
        self.qlayer = QuantumLayer(n_qubits, n_layers, backend, shots, diff_method, noise, trajectories)
        self.preprocess = nn.Sequential(
            nn.Conv2d(2, 16, kernel_size=3, stride=1, padding=1),
            nn.ReLU(),
            nn.MaxPool2d(2),
            nn.Conv2d(16, 32, kernel_size=3, stride=1, padding=1),
            nn.ReLU(),
            nn.MaxPool2d(2),
            nn.Flatten(),
            nn.Linear(flat, n_qubits),
            nn.Tanh(),
        )
        self.classifier = nn.Linear(n_qubits, n_classes)
        if not use_quantum:
            self.classical_fallback = nn.Sequential(nn.Linear(n_qubits, n_qubits), nn.Tanh())
        if post_norm:   # (last: the keys before it are those of the default model, in its order)
            self.postmeas = PostMeasurement(n_qubits, int(post_quant_levels), float(post_quant_range),
                                            float(post_quant_weight))

    def post_config(self) -> dict:
        """The post-measurement arguments this model was built with (checkpoint meta)."""
        pm = getattr(self, "postmeas", None)
        if pm is None:
            return {}
        return {"post_norm": True, "post_quant_levels": pm.levels, "post_quant_range": pm.qrange,
                "post_quant_weight": pm.weight}

    def quantum_weights(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        w = self.qlayer.weights
        if self.training and self.use_quantumnat and self.noise_level > 0:
            noise = torch.randn(w.shape, device=w.device, dtype=w.dtype, generator=generator)
            return w + self.noise_level * noise
        return w

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        angles = self.preprocess(x)
        if self.use_quantum:
            xq = self.qlayer(angles, self.quantum_weights())
        else:
            xq = self.classical_fallback(angles)
        if getattr(self, "postmeas", None) is not None:
            xq = self.postmeas(xq)
        return F.log_softmax(self.classifier(xq), dim=1)

    @torch.no_grad()
    def apply_gradient_pruning(self, sync_stats: bool = True) -> None:
        """g *= (|g| > threshold) for every parameter (E:205-228)."""
        if not self.use_gradient_pruning:
            return
        total, pruned = 0, None
        for p in self.parameters():
            if p.grad is None:
                continue
            mask = p.grad.abs() > self.gradient_threshold
            cnt = (~mask).sum()
            pruned = cnt if pruned is None else pruned + cnt
            total += p.grad.numel()
            p.grad.mul_(mask)
        if sync_stats and total > 0 and pruned is not None:
            ratio = pruned.item() / total
            self.last_pruning_ratio = ratio
            if ratio > 0.1:
                print(f"Gradient pruning: {ratio:.1%} gradients pruned")


class Conv_P128(nn.Module):
    """Per-scenario feature extractor (E:237-268): (B,2,H,W) -> (B, 32*H*W), C-major flatten."""

    def __init__(self, pilot_num: int = 128):
        super().__init__()
        self.features, self.kernel_size, self.padding = 32, 3, 1
        self.H, self.W = pilot_grid(pilot_num)
        self.cnn = _cnn_stack(self.features, self.kernel_size, self.padding)

    def forward(self, x):
        x = self.cnn(x)
        return x.reshape(x.shape[0], self.features * self.H * self.W)


class FC_P128(nn.Module):
    """Shared feature mapper Linear(32*H*W -> 2048) (E:272-279)."""

    def __init__(self, pilot_num: int = 128, out_dim: int = 64 * 16 * 2):
        super().__init__()
        H, W = pilot_grid(pilot_num)
        self.FC = nn.Linear(32 * H * W, out_dim)

    def forward(self, x):
        return self.FC(x)


def NMSE_cuda(x_hat: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Batch-global NMSE: sum((x_hat-x)^2) / sum(x^2) over the WHOLE tensor (E:282-286)."""
    x_hat = x_hat.float()
    x = x.float()
    return torch.sum((x_hat - x) ** 2) / torch.sum(x ** 2)


class NMSELoss(nn.Module):
    def forward(self, x_hat, x):
        return NMSE_cuda(x_hat, x)
