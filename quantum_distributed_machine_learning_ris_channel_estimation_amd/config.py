"""Typed configuration for the framework.

The reference hard-codes its knobs as attributes of ``Y2HRunner.__init__``
(Runner_P128_QuantumNAT_onchipQNN.py:20-33) and ``model_val.__init__``
(Test.py:14-21); QSC constructor knobs live at
Estimators_QuantumNAT_onchipQNN.py:108-119.  We keep *the same attribute names*
so existing user code that pokes ``runner.lr = ...`` keeps working, and add the
MI355X-specific knobs (world size, dtype, qubits, HIP graphs, bucket sizes).

Overrides come from ``update_from_dict`` (CLI ``--set key=value`` or a
YAML/JSON file via ``load_config_file``).
"""
from __future__ import annotations

import dataclasses
import json
import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional


@dataclass
class RunnerConfig:
    # --- reference knobs (R:20-33) -------------------------------------------------
    Pilot_num: int = 128
    data_len: int = 20000
    SNRdb: int = 10
    num_workers: int = 0
    batch_size: int = 256          # unused by the reference (R:25); kept for parity
    batch_size_DML: int = 256      # per-stream batch (R:26)
    lr: float = 1e-3
    lr_decay: int = 30             # epochs between x0.5 LR steps (HDCE, R:272-283)
    lr_threshold: float = 1e-6     # LR floor (R:279)
    n_epochs: int = 100
    print_freq: int = 50
    optimizer: str = "adam"        # 'adam' | 'sgd' (R:40-46)
    train_test_ratio: float = 0.9

    # --- QSC constructor knobs (E:108, runner passes False/False at R:313-316) -----
    n_qubits: int = 6
    n_layers: int = 3
    n_classes: int = 3
    use_quantumnat: bool = False
    use_gradient_pruning: bool = False
    noise_level: float = 0.01       # E:118
    gradient_threshold: float = 0.1  # E:119
    qsc_weight_decay: float = 0.01   # AdamW wd (R:320)

    # --- framework knobs (new) -----------------------------------------------------
    n_scenarios: int = 3
    n_users: int = 3
    workspace: str = "./workspace"
    data_dir: str = "available_data"
    synthetic: bool = True          # generate DeepMIMO-shaped data when .npy files are absent
    seed: int = 0
    dtype: str = "bf16"             # estimator compute dtype: fp32 | bf16
    hdce_engine: str = "hip"        # HDCE training step: hip (fused kernels, bf16 MFMA) | torch (autograd; with
    #                                 dtype fp32: an all-fp32 reference run of the same step, FIG1 attribution)
    device: str = "auto"            # auto | cuda | cpu
    backend: str = "auto"           # kernel backend: auto | hip | cpu | torch
    hip_graphs: bool = True
    dp_graphs: str = "auto"         # N > 1 with RCCL: capture each training step -- its bucketed all-reduces
    #                                 included -- in a HIP graph (on | off | auto: on when the entry point's
    #                                 capture pre-flight, parallel/capture_probe.py, passed on every rank)
    overlap_comm: bool = True
    bucket_mb: float = 32.0
    world_size: int = 1
    dp_semantics: str = "weak"      # N > 1: weak (every rank runs batch_size_DML per stream on its own data shard:
    #                                 the benchmark's weak scaling) | reference (DataParallel's split: one global
    #                                 batch of batch_size_DML per stream cut into world parts, global NMSE
    #                                 denominators, per-replica BatchNorm -- R:144-148)
    log_jsonl: Optional[str] = None
    deterministic: bool = False
    nan_guard: bool = True
    resume: bool = False
    # HDCE weight averaging: the mean of the estimator's weights over the last ``swa_epochs`` epochs (one snapshot
    # per epoch end), with every expert's BN statistics re-estimated on its training streams, saved beside the
    # epoch checkpoints under the tag "swa" (0: off; the reference evaluates the last epoch's weights)
    swa_epochs: int = 0
    # on-chip QSC training (train-qsc; EvalConfig's names): the backward of the quantum layer (ops/quantum.py
    # DIFF_METHODS: adjoint | parameter_shift | on_chip | noisy_adjoint), the measurement shots per circuit (0: exact), and the
    # device noise the shots are measured under (needs qsc_shots > 0): Pauli error rate per fused one-qubit gate /
    # per CNOT, readout error 0 -> 1 / 1 -> 0, gate-error realisations the shots are split over.  Anything but the
    # defaults trains through the module path (no fused step, no graph capture), world size 1 only.
    qsc_diff_method: str = "adjoint"
    qsc_shots: int = 0
    qsc_noise_p1: float = 0.0
    qsc_noise_p2: float = 0.0
    qsc_readout01: float = 0.0
    qsc_readout10: float = 0.0
    qsc_trajectories: int = 1
    # qsc_noise_exact: the rates act through the exact channel instead -- the density matrix of ops/quantum.py
    # qsim_mixed, no shots and no trajectories (qsc_shots == 0, n_qubits <= 8, gate rates <= 0.5), differentiated by
    # its one-launch adjoint; in the module path or (qsc_step=fused) the fused, graphed step
    qsc_noise_exact: bool = False
    # qsc_step: where those modes train -- "module" (the default: the path above) or "fused": the fused, graph-captured
    # step (ops/qsc.py QSCStepHIP's measured modes; on a CPU device the module path).  QOC gradient pruning
    # (ops/qoc.py; needs parameter_shift or on_chip, either path): after every qsc_prune_accum steps that measure all
    # parameters, qsc_prune_window steps measure only a sampled (1 - qsc_prune_ratio) of them (0: off)
    qsc_step: str = "module"
    qsc_prune_ratio: float = 0.0
    qsc_prune_accum: int = 1
    qsc_prune_window: int = 2
    # QuantumNAT post-measurement processing of the QSC's measured <Z_j> (models/estimators.py PostMeasurement, off by
    # default; qsc_step=module and fused alike, world size 1 only): per-wire normalization over the step's batch, and
    # with qsc_post_quant_levels >= 2 (needs qsc_post_norm) quantization to that many levels on +-qsc_post_quant_range
    # with the quadratic penalty qsc_post_quant_weight * mean (z - Q)^2 in the loss
    qsc_post_norm: bool = False
    qsc_post_quant_levels: int = 0
    qsc_post_quant_range: float = 2.0
    qsc_post_quant_weight: float = 0.0
    # quantum natural gradient (ops/qng.py, off by default; train-qsc on either qsc_step, any measurement mode, world
    # size 1 only): before AdamW sees it, every (layer, RY | RZ) block of the quantum layer's gradient is solved
    # against (g + qsc_qng_lambda I), g the block-diagonal Fubini-Study metric of the noiseless circuit at the clean
    # master weights, averaged over the step's samples.  The QOC pruner still accounts the raw gradient.
    qsc_qng: bool = False
    qsc_qng_lambda: float = 0.01

    def update_from_dict(self, d: Dict[str, Any]) -> "RunnerConfig":
        names = {f.name: f for f in dataclasses.fields(self)}
        for k, v in d.items():
            if k not in names:
                raise KeyError(f"unknown config key {k!r}")
            setattr(self, k, _coerce(v, type(getattr(self, k))))
        return self

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)


@dataclass
class EvalConfig:
    # --- reference knobs (T:14-21, T:66) ----------------------------------------------
    training_SNRdb: int = 10
    num_workers: int = 8
    batch_size: int = 200
    batch_size_DML: int = 256
    training_data_len: int = 20000
    indicator: int = -1
    data_len_for_test: int = 10000
    Pilot_num: int = 128
    snr_list: tuple = (5, 7, 9, 11, 13, 15)
    # framework knobs
    workspace: str = "./workspace"
    results_dir: str = "results"
    n_qubits: int = 6
    n_layers: int = 3
    seed: int = 1234
    device: str = "auto"
    backend: str = "auto"
    # test-time BN adaptation: re-estimate each expert's BN statistics on the test pilots routed to it
    # (unsupervised; the reference keeps the 10 dB training statistics -- reports/r2_hdce_snr.md)
    bn_adapt: bool = False
    # the HDCE checkpoint tag to evaluate ("": the classifiers' epoch tag; "swa": RunnerConfig.swa_epochs' average)
    hdce_tag: str = ""
    # measurement shots per sample of the quantum SC's circuit (0: exact expectation values; ops/quantum.py qsim)
    qsc_shots: int = 0
    # the device noise those shots are measured under (used only with qsc_shots > 0; ops/quantum.py NoiseModel):
    # Pauli error rate per fused one-qubit gate / per CNOT, readout error 0 -> 1 / 1 -> 0, and the number of gate-
    # error realisations the shots are split over
    qsc_noise_p1: float = 0.0
    qsc_noise_p2: float = 0.0
    qsc_readout01: float = 0.0
    qsc_readout10: float = 0.0
    qsc_trajectories: int = 1
    # True: the rates above are evaluated exactly -- the expectation of the noisy device itself, the density matrix of
    # ops/quantum.py qsim_mixed (n_qubits <= 8), with no shots and no trajectories: needs qsc_shots == 0
    qsc_noise_exact: bool = False
    # a quantum SC trained with post-measurement normalization (its checkpoint says so): normalize with the statistics
    # of the evaluated chunk itself ("batch": removes a noisy device's per-wire affine distortion, but a prediction
    # then depends on the chunk it is in) or with the running statistics of training ("running")
    qsc_post_stats: str = "batch"
    # test-time routing: "hard" (the reference: every sample through the arg-max expert of the classifier) or
    # "soft" (additionally: the experts combined under the classifier's posterior, and the oracle routing by the true
    # scenario -- the nmse_*_soft / nmse_oracle rows)
    routing: str = "hard"
    # precision of the shared FC at test time: "bf16", or "fp8" -- OCP e4m3 with one power-of-two scale per operand
    # row (sample, expert) and per output channel (no calibration; the precision the fp8 estimator is trained in)
    dtype: str = "bf16"

    def update_from_dict(self, d: Dict[str, Any]) -> "EvalConfig":
        names = {f.name for f in dataclasses.fields(self)}
        for k, v in d.items():
            if k not in names:
                raise KeyError(f"unknown config key {k!r}")
            cur = getattr(self, k)
            setattr(self, k, tuple(v) if isinstance(cur, tuple) else _coerce(v, type(cur)))
        return self


def _coerce(v: Any, ty: type) -> Any:
    if v is None or ty is type(None):
        return v
    if isinstance(v, str) and ty is not str:
        if ty is bool:
            return v.lower() in ("1", "true", "yes", "on")
        return ty(v)
    if ty is float and isinstance(v, int):
        return float(v)
    return v


def load_config_file(path: str) -> Dict[str, Any]:
    """Load a YAML (safe loader only) or JSON override file."""
    with open(path, "r") as f:
        text = f.read()
    if path.endswith((".yaml", ".yml")):
        import yaml
        return yaml.safe_load(text) or {}
    return json.loads(text)


def parse_overrides(items) -> Dict[str, Any]:
    """``["lr=1e-3", "n_qubits=8"]`` -> dict (values parsed as JSON when possible)."""
    out: Dict[str, Any] = {}
    for it in items or []:
        k, _, v = it.partition("=")
        try:
            out[k] = json.loads(v)
        except json.JSONDecodeError:
            out[k] = v
    return out


def resolve_device(device: str = "auto"):
    import torch
    if device == "auto":
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device(device)


def env_rank_info():
    """torchrun-compatible rank discovery (RANK / WORLD_SIZE / LOCAL_RANK)."""
    return (int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)),
            int(os.environ.get("LOCAL_RANK", 0)))
