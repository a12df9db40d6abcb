"""``model_val``: NMSE-vs-SNR + scenario-classification evaluation (reference: Test.py).

Reference flow (Test.py:64-275): load the classical SC (``{bs}_{snr}dB_epoch99_DML_SC.pth``,
key 'cnn'), the quantum SC (``QSC_optimized_best.pth``, key 'model_state_dict', dropped
silently on failure), Conv0-2 and the shared Linear (``*_epoch99_DML.pth``); for each test
SNR in 5:2:15 dB generate 10k mixed-scenario samples, compute the LS and MMSE baselines,
classify every sample (classical and quantum), route it to ``Conv_{pred}`` then the shared
CE, and report global NMSE vs the perfect channel and SC accuracy; plot + JSON.

Differences by design (MI355X): the test set is generated directly on the device, routing
is one sort + per-expert batches (no per-sample Python loop, Test.py:166-179), the MMSE
is a complex GEMM on the device, and nothing goes through an 8-worker host DataLoader.
The quantum classifier is built from the checkpoint's own ``qsc_config`` (the reference
binds the class instead of an instance, T:77 -- a bug we do not reproduce).
"""
from __future__ import annotations

import glob
import json
import os
import re
from typing import Dict, List, Optional

import numpy as np
import torch

from ..config import EvalConfig, resolve_device
from ..data.baselines import lmmse_estimate
from ..data.channel import generate_mixed, pack_channel, pack_pilots
from ..models.estimators import Conv_P128, FC_P128, NMSELoss, QSC_P128, SC_P128
from . import checkpoint as ck
from .engine import INFER_DTYPES, estimate_mixed, estimate_routed


@torch.no_grad()
def recalibrate_bn(convs, x: torch.Tensor, expert: torch.Tensor, chunk: int = 4096) -> list:
    """Re-estimate every expert's BN running statistics (cumulative average over the inputs routed to it);
    returns the previous statistics for ``restore_bn``.  An expert that receives no input keeps its own."""
    saved = []
    for e, conv in enumerate(convs):
        bns = [m for m in conv.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        saved.append([(m.momentum, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone())
                      for m in bns])
        xe = x[expert == e]
        if xe.shape[0] < 2:
            continue
        for m in bns:
            m.reset_running_stats()
            m.momentum = None
        was = conv.training
        conv.train()
        for s in range(0, xe.shape[0], chunk):
            if xe.shape[0] - s >= 2:
                conv(xe[s:s + chunk].float())
        conv.train(was)
    return saved


@torch.no_grad()
def restore_bn(convs, saved: list) -> None:
    for conv, st in zip(convs, saved):
        bns = [m for m in conv.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        for m, (mom, rm, rv, nb) in zip(bns, st):
            m.momentum = mom
            m.running_mean.copy_(rm)
            m.running_var.copy_(rv)
            m.num_batches_tracked.copy_(nb)


def _epoch_file(d: str, pattern_fmt: str, prefer: str) -> Optional[str]:
    """The reference hard-codes 'epoch99'; fall back to the latest epoch present."""
    p = os.path.join(d, pattern_fmt.format(tag=prefer))
    if os.path.exists(p):
        return p
    best, best_e = None, -1
    rx = re.compile(re.escape(pattern_fmt.format(tag="epoch@")).replace("@", r"(\d+)"))
    for f in glob.glob(os.path.join(d, pattern_fmt.format(tag="epoch*"))):
        m = rx.search(os.path.basename(f))
        if m and int(m.group(1)) > best_e:
            best, best_e = f, int(m.group(1))
    return best


ROUTINGS = ("hard", "soft")
SOFT_KEYS = ("nmse_classical_soft", "nmse_quantum_soft", "nmse_oracle")   # evaluate_snr's extra rows of "soft"


class model_val:
    def __init__(self, cfg: Optional[EvalConfig] = None, **overrides):
        cfg = cfg or EvalConfig()
        if overrides:
            cfg.update_from_dict(overrides)
        self.cfg = cfg
        for k, v in vars(cfg).items():
            setattr(self, k, v)
        self.device = resolve_device(cfg.device)
        self.epoch_tag = "epoch99"
        self.hip_engine = True   # (GPU) the HIP inference engine; False: the models' torch forward
        self._qsc_noise = None
        self.qsc_noise_model()   # (refuses noise rates without qsc_shots)
        self._post_stats()
        self._routing()
        self._dtype()
        self.results: Dict[str, List[float]] = {}

    def load_model_state_dict(self, model, filepath, fallback_key=None):
        ck.load_model_state_dict(model, filepath, fallback_key, map_location=self.device)

    def qsc_noise_model(self):
        """The ``NoiseModel`` of the qsc_noise_* / qsc_readout* knobs (None: all rates zero); it needs qsc_shots, or
        qsc_noise_exact (the exact channel, which takes no shots)."""
        rates = (float(self.qsc_noise_p1), float(self.qsc_noise_p2), float(self.qsc_readout01),
                 float(self.qsc_readout10))
        exact = bool(getattr(self, "qsc_noise_exact", False))
        if exact and int(self.qsc_shots) > 0:
            raise ValueError("qsc_noise_exact evaluates the noisy device's expectation itself: it needs qsc_shots == 0")
        if not any(rates):
            return None
        if int(self.qsc_shots) <= 0 and not exact:
            raise ValueError("qsc_noise_* / qsc_readout* need qsc_shots > 0: the noise model is sampled per shot")
        if self._qsc_noise is None or self._qsc_noise[0] != rates:
            from ..ops.quantum import NoiseModel
            self._qsc_noise = (rates, NoiseModel(*rates))
        return self._qsc_noise[1]

    def _post_stats(self) -> str:
        from ..ops.postmeas import STATS
        if str(self.qsc_post_stats) not in STATS:
            raise ValueError(f"unknown qsc_post_stats {self.qsc_post_stats!r}: one of {STATS}")
        return str(self.qsc_post_stats)

    def _routing(self) -> str:
        if self.routing not in ROUTINGS:
            raise ValueError(f"unknown routing {self.routing!r}: one of {ROUTINGS}")
        return self.routing

    def _dtype(self) -> str:
        if self.dtype not in INFER_DTYPES:
            raise ValueError(f"unknown dtype {self.dtype!r}: one of {INFER_DTYPES}")
        return self.dtype

    # ------------------------------------------------------------------ loading
    def _dir(self) -> str:
        return ck.ckpt_dir(self.workspace, self.Pilot_num, make=False)

    def load_qsc(self, fq: str) -> QSC_P128:
        """The quantum SC of checkpoint ``fq``, built from its own ``qsc_config`` meta (a checkpoint without the
        post-measurement keys loads as a plain QSC); a PostMeasurement module evaluates with ``qsc_post_stats``."""
        dev = self.device
        meta = torch.load(fq, map_location="cpu", weights_only=True).get("qsc_config", {})
        post = {k: meta[k] for k in ("post_norm", "post_quant_levels", "post_quant_range", "post_quant_weight")
                if k in meta}
        qsc = QSC_P128(meta.get("n_qubits", self.n_qubits), meta.get("n_layers", self.n_layers),
                       meta.get("n_classes", 3), use_quantumnat=False, use_gradient_pruning=False,
                       pilot_num=self.Pilot_num, backend=None if self.backend == "auto" else self.backend,
                       **post).to(dev)
        if getattr(qsc, "postmeas", None) is not None:
            qsc.postmeas.stats = self._post_stats()
        self.load_model_state_dict(qsc, fq, fallback_key="model_state_dict")
        return qsc

    def load_models(self):
        d, bs, snr = self._dir(), self.batch_size_DML, self.training_SNRdb
        dev = self.device
        sc = SC_P128(self.Pilot_num).to(dev)
        f = _epoch_file(d, f"{bs}_{snr}dB_{{tag}}_DML_SC.pth", self.epoch_tag)
        if f is None:
            raise FileNotFoundError(f"classical SC checkpoint not found in {d}")
        self.load_model_state_dict(sc, f, fallback_key="cnn")
        qsc = None
        fq = os.path.join(d, "QSC_optimized_best.pth")
        try:
            qsc = self.load_qsc(fq)
        except Exception as e:  # reference: bare except -> classical only (T:81-86)
            print(f"Quantum SC model not found, using classical only ({type(e).__name__})")
            qsc = None
        convs = [Conv_P128(self.Pilot_num).to(dev) for _ in range(3)]
        fc = FC_P128(self.Pilot_num).to(dev)
        htag = self.hdce_tag or self.epoch_tag
        for name, model, key in [("Conv0", convs[0], "conv"), ("Conv1", convs[1], "conv"),
                                 ("Conv2", convs[2], "conv"), ("Linear", fc, "linear")]:
            f = (_epoch_file(d, f"{name}_{bs}_{snr}dB_{{tag}}_DML.pth", htag) if htag.startswith("epoch")
                 else os.path.join(d, f"{name}_{bs}_{snr}dB_{htag}_DML.pth"))
            if not os.path.exists(f or ""):
                f = None
            if f is None:
                raise FileNotFoundError(f"{name} checkpoint not found in {d}")
            self.load_model_state_dict(model, f, fallback_key=key)
        for m in [sc, fc] + convs + ([qsc] if qsc is not None else []):
            m.eval()
        return sc, qsc, convs, fc

    # ------------------------------------------------------------------ sweep
    @torch.no_grad()
    def evaluate_snr(self, snr: float, sc, qsc, convs, fc, chunk: int = 4096) -> Dict[str, float]:
        dev = self.device
        criterion = NMSELoss()
        self.qsc_noise_model()   # (a noise rate without qsc_shots is an error, not a silently exact sweep)
        Yp, HLS, H, ind = generate_mixed(self.data_len_for_test, float(snr), self.Pilot_num, self.indicator,
                                         base_seed=self.seed, split=f"test@{self.training_data_len * 3}", device=dev)
        # FIG1's "MMSE" row: the reference-calibrated subspace estimator (~LS - 1.3 dB at every SNR, the
        # reference's published gap); the per-subcarrier Wiener LMMSE is reported alongside
        HMMSE = lmmse_estimate(HLS, 10 ** (-snr / 10), mode="subspace")
        HLMMSE = lmmse_estimate(HLS, 10 ** (-snr / 10), mode="freq")
        perf = pack_channel(H)
        x = pack_pilots(Yp, self.Pilot_num)
        out = {"nmse_ls": float(criterion(pack_channel(HLS), perf)),
               "nmse_mmse": float(criterion(pack_channel(HMMSE), perf)),
               "nmse_lmmse": float(criterion(pack_channel(HLMMSE), perf))}
        soft = self._routing() == "soft"
        dt = self._dtype()   # ("fp8": the shared FC in e4m3 -- the engine's kernels, or engine.py's torch definition)
        if soft:
            for clf in (sc, qsc):
                nc = None if clf is None else clf.FC.out_features if isinstance(clf, SC_P128) else clf.n_classes
                if nc is not None and nc != len(convs):
                    raise ValueError(f"soft routing: a classifier of {nc} classes cannot weight {len(convs)} experts")
        eng = self._hip_engine(sc, qsc, convs, fc)
        if soft:   # the oracle row: hard routing by the true scenario
            Hor = eng.estimate(x, ind) if eng is not None else estimate_routed(convs, fc, x, ind.to(x.device), dtype=dt)
            out["nmse_oracle"] = float(criterion(Hor, perf))
        for tag, clf in (("classical", sc), ("quantum", qsc)):
            if clf is None:
                out[f"nmse_{tag}"], out[f"acc_{tag}"] = float("nan"), float("nan")
                if soft:
                    out[f"nmse_{tag}_soft"] = float("nan")
                continue
            # qsc_shots > 0: the quantum SC's circuit is measured with that many shots per sample (seeded by cfg.seed)
            shots = int(self.qsc_shots) if tag == "quantum" and getattr(clf, "use_quantum", False) else 0
            # qsc_noise_exact: the rates act through the exact channel (ops/quantum.py qsim_mixed), without shots
            exact = (bool(self.qsc_noise_exact) and tag == "quantum" and getattr(clf, "use_quantum", False)
                     and self.qsc_noise_model() is not None)
            noise = self.qsc_noise_model() if shots or exact else None
            traj = int(self.qsc_trajectories) if noise is not None and not exact else 1
            if eng is not None and (eng.sc if tag == "classical" else eng.qsc) is not None:
                # the HIP kernels: classifier, experts, routed FC (train/infer.py)
                if exact:
                    pred = eng.classify(x, tag, noise=noise, exact_noise=True, return_logp=soft)
                else:
                    pred = (eng.classify(x, tag, shots=shots, seed=self.seed, noise=noise, trajectories=traj,
                                         return_logp=soft) if shots else eng.classify(x, tag, return_logp=soft))
                pred, logp = pred if soft else (pred, None)
            else:   # (CPU, or the classical-fallback QSC ablation: torch)
                if exact:
                    ql = clf.qlayer
                    plain = (ql.shots, ql.noise, ql.exact_noise)
                    ql.shots, ql.noise, ql.exact_noise = None, noise, True
                if shots:
                    ql = clf.qlayer
                    saved_ql = (ql.shots, ql.shot_seed, ql._shot_calls, ql.noise, ql.trajectories)
                    ql.shots, ql.noise, ql.trajectories = shots, noise, traj
                    ql.manual_shot_seed(self.seed)
                try:
                    logp = torch.cat([clf(x[i:i + chunk]) for i in range(0, x.shape[0], chunk)])
                    pred = logp.argmax(1)
                finally:
                    if shots:
                        ql.shots, ql.shot_seed, ql._shot_calls, ql.noise, ql.trajectories = saved_ql
                    if exact:
                        ql.shots, ql.noise, ql.exact_noise = plain
            saved = None
            if self.bn_adapt:   # (GPU: the HIP training conv forward computes the statistics, no MIOpen)
                saved = eng.recalibrate_bn(convs, x, pred) if eng is not None else recalibrate_bn(convs, x, pred)
            if eng is not None:
                if saved is not None:
                    eng.load_bn_stats(convs)
                Hhat = eng.estimate(x, pred)
            else:
                Hhat = estimate_routed(convs, fc, x, pred, dtype=dt)
            if soft:   # the experts under the posterior the prediction was the arg-max of (same shots, noise, seed)
                wts = logp.float().exp()
                Hs = eng.estimate_mixed(x, wts) if eng is not None else estimate_mixed(convs, fc, x, wts, dtype=dt)
                out[f"nmse_{tag}_soft"] = float(criterion(Hs, perf))
            if saved is not None:
                restore_bn(convs, saved)
                if eng is not None:
                    eng.load_bn_stats(convs)   # (the engine keeps copies: hand the restored statistics back)
            out[f"nmse_{tag}"] = float(criterion(Hhat, perf))
            out[f"acc_{tag}"] = float((pred == ind).float().mean())
        return out

    def _hip_engine(self, sc, qsc, convs, fc):
        """The HIP inference engine for these models (GPU; None on the CPU, or with ``hip_engine`` off)."""
        if self.device.type != "cuda" or not self.hip_engine:
            return None
        # the engine keeps COPIES of the weights: key it on the modules themselves (strong references, so a
        # freed module's id can never be reused by a later model) and on the version counter of every
        # parameter (an in-place update -- more training, a load_state_dict -- rebuilds it; BN statistics
        # the sweep itself adapts are handed over by load_bn_stats)
        mods = [m for m in (sc, qsc, *convs, fc) if m is not None]
        ver = tuple(t._version for m in mods for t in m.parameters())
        key = (tuple(mods), ver, self._dtype())
        old = getattr(self, "_eng_key", None)
        if old is None or len(old[0]) != len(key[0]) or any(a is not b for a, b in zip(old[0], key[0])) \
                or old[1:] != key[1:]:
            from .infer import HIPInference
            self._eng = HIPInference(convs, fc, self.Pilot_num, self.device, sc=sc,
                                     qsc=qsc if (qsc is not None and qsc.use_quantum) else None, dtype=key[2])
            self._eng_key = key
        return self._eng

    def test_for_CE_P128_for_all_scenarios(self):
        sc, qsc, convs, fc = self.load_models()
        SNRdb = np.array(self.snr_list)
        keys = ["nmse_ls", "nmse_mmse", "nmse_lmmse", "nmse_classical", "nmse_quantum", "acc_classical", "acc_quantum"]
        res = {k: [] for k in keys}
        for snr in SNRdb:
            print(f"Generating test data for SNR: {snr} dB")
            r = self.evaluate_snr(float(snr), sc, qsc, convs, fc)
            for k in keys:
                res[k].append(r[k])
            for k in SOFT_KEYS:   # (routing="soft")
                if k in r:
                    res.setdefault(k, []).append(r[k])
            db = lambda v: 10 * np.log10(v)
            print(f"SNR {snr}dB Results:")
            print(f"  LS NMSE: {db(r['nmse_ls']):.2f} dB")
            print(f"  MMSE NMSE: {db(r['nmse_mmse']):.2f} dB")
            print(f"  LMMSE NMSE: {db(r['nmse_lmmse']):.2f} dB")
            print(f"  HDCE (Classical) NMSE: {db(r['nmse_classical']):.2f} dB")
            if qsc is not None:
                print(f"  HDCE (Quantum) NMSE: {db(r['nmse_quantum']):.2f} dB")
            print(f"  SC Accuracy (Classical): {r['acc_classical']:.4f}")
            if qsc is not None:
                print(f"  SC Accuracy (Quantum): {r['acc_quantum']:.4f}")
            for k in SOFT_KEYS:
                if k in r and r[k] == r[k]:
                    print(f"  {k}: {db(r[k]):.2f} dB")
        self.results = res
        self.create_comparison_plots(SNRdb, res["nmse_ls"], res["nmse_mmse"], res["nmse_classical"],
                                     res["nmse_quantum"], res["acc_classical"], res["acc_quantum"],
                                     nmse_lmmse=res["nmse_lmmse"], soft={k: res[k] for k in SOFT_KEYS if k in res})
        return 0

    # ------------------------------------------------------------------ reporting
    def create_comparison_plots(self, SNRdb, nmse_ls, nmse_mmse, nmse_classical, nmse_quantum, acc_classical,
                                acc_quantum, nmse_lmmse=None, soft=None):
        os.makedirs(self.results_dir, exist_ok=True)
        db = lambda xs: [10 * np.log10(x) if x == x else float("nan") for x in xs]
        results = {
            "SNR_dB": [int(s) for s in SNRdb],
            "NMSE_LS_dB": db(nmse_ls),
            "NMSE_MMSE_dB": db(nmse_mmse),
            "NMSE_HDCE_Classical_dB": db(nmse_classical),
            "NMSE_HDCE_Quantum_dB": db(nmse_quantum),
            "Accuracy_Classical": list(map(float, acc_classical)),
            "Accuracy_Quantum": list(map(float, acc_quantum)),
            "qsc_shots": int(self.qsc_shots),   # (0: exact expectation values)
            "qsc_noise_p1": float(self.qsc_noise_p1), "qsc_noise_p2": float(self.qsc_noise_p2),
            "qsc_readout01": float(self.qsc_readout01), "qsc_readout10": float(self.qsc_readout10),
            "qsc_trajectories": int(self.qsc_trajectories),
            "qsc_noise_exact": bool(self.qsc_noise_exact),   # (True: the rates through the exact channel, no shots)
        }
        if nmse_lmmse is not None:
            results["NMSE_LMMSE_dB"] = db(nmse_lmmse)
        for k, v in (soft or {}).items():   # routing="soft": NMSE_HDCE_Classical_Soft_dB, ..._Quantum_Soft_dB, ..._Oracle_dB
            results["NMSE_HDCE_" + "_".join(w.capitalize() for w in k.split("_")[1:]) + "_dB"] = db(v)
        with open(os.path.join(self.results_dir, "quantum_classical_comparison.json"), "w") as f:
            json.dump(results, f, indent=4)
        try:
            from ..utils.plots import plot_fig1
            plot_fig1(results, os.path.join(self.results_dir, "Quantum_vs_Classical_Comparison.png"))
        except Exception as e:  # plotting is optional (headless boxes)
            print(f"plot skipped: {e}")
        print(f"Results saved to '{os.path.join(self.results_dir, 'quantum_classical_comparison.json')}'")
        return results
