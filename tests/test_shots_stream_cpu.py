"""Finite-shot measurement above 12 qubits on the host: the wide sampler of csrc/cpu/qsim_cpu.cpp
(qd_cpu_sample_z_wide, 2 <= n <= 16: the oracle of csrc/hip/qsim_stream_shots.hip) against an independent NumPy
implementation of the sampling contract stated in csrc/hip/qsim_shots.hip, degenerate rows around the 4096-outcome
block boundary, the statistical bound of ``qsim(shots=)`` at n = 13 and 16, and the unchanged n <= 12 path."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.quantum import qsim, sample_z, z_signs

from test_shots_cpu import CPU, SEED, _philox, inputs, shot_bound

SEED_HI = 0x9E3779B97F4A7C15          # non-zero high word
CTR_HI = (1 << 32) + (1 << 40) + 77   # above 2^32
STAT_CASES = [(13, 2, 2), (16, 3, 2), (13, 2, 3), (16, 3, 3)]   # (B = 3: the inputs of the GPU file's bound)


def contract_counts(p: torch.Tensor, shots: int, seed: int, ctr: int):
    """(E, counts) of the sampling contract, from its statement alone: q = rint(p 2^30) (fp32 product, to nearest
    even), the uint32 inclusive prefix sum, Philox word (s & 3) of counter (s >> 2, row, lo(ctr), hi(ctr)),
    t = (r T) >> 32, outcome = the first index with cum > t (an all-zero row: D - 1)."""
    B, D = p.shape
    n = D.bit_length() - 1
    pf = p.numpy().astype(np.float32)
    q = np.where(pf > 0, np.rint(pf * np.float32(2.0 ** 30)), 0).astype(np.uint32)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    counts = np.zeros((B, n), dtype=np.int32)
    for b in range(B):
        cum = np.cumsum(q[b], dtype=np.uint32)
        T = int(cum[-1])
        words = []
        for j in range((shots + 3) // 4):
            words += _philox([j, b, ctr & 0xFFFFFFFF, (ctr >> 32) & 0xFFFFFFFF], key)
        t = (np.array(words[:shots], dtype=np.uint64) * np.uint64(T)) >> np.uint64(32)
        k = np.minimum(np.searchsorted(cum, t.astype(np.uint32), side="right"), D - 1)
        for i in range(n):
            counts[b, i] = int(((k >> i) & 1).sum())
    E = (np.float32(shots) - 2 * counts.astype(np.float32)) / np.float32(shots)   # (exact integers below 2^24)
    return torch.from_numpy(E.astype(np.float32)), torch.from_numpy(counts)


@pytest.mark.parametrize("n", [13, 14, 16])
def test_wide_sampler_matches_the_contract(n):
    B, D = 2, 1 << n
    p = torch.rand(B, D, generator=torch.Generator().manual_seed(n))
    p = (p / p.sum(1, keepdim=True)).float()
    for shots in (1, 63, 65, 257):
        E, c = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
        Er, cr = contract_counts(p, shots, SEED_HI, CTR_HI)
        assert torch.equal(c, cr), (n, shots)
        assert torch.equal(E, Er), (n, shots)


def degenerate_rows(n: int) -> torch.Tensor:
    """One-hot rows at 0, D - 1, 4095 and 4096, a row with mass at odd indices only, an all-zero row."""
    D = 1 << n
    p = torch.zeros(6, D)
    for b, k in enumerate((0, D - 1, 4095, 4096)):
        p[b, k] = 1.0
    p[4, 1::2] = torch.rand(D // 2, generator=torch.Generator().manual_seed(1)) + 0.1
    p[4] /= p[4].sum()
    return p


def check_degenerate(n: int, shots: int, E: torch.Tensor, c: torch.Tensor) -> None:
    D = 1 << n
    for b, k in enumerate((0, D - 1, 4095, 4096)):
        assert torch.equal(E[b], z_signs(n)[k]), (n, shots, k)
    assert float(E[4, 0]) == -1.0 and int(c[4, 0]) == shots
    assert torch.equal(c[5], torch.full((n,), shots, dtype=torch.int32))   # all zero: outcome D - 1
    assert torch.equal(E[5], -torch.ones(n))


@pytest.mark.parametrize("n", [13, 16])
@pytest.mark.parametrize("shots", [1, 63, 257])
def test_degenerate_distributions_wide(n, shots):
    E, c = sample_z(degenerate_rows(n), shots, seed=SEED, return_counts=True)
    check_degenerate(n, shots, E, c)


@pytest.mark.parametrize("n,L,B", STAT_CASES)
def test_statistical_bound_wide(n, L, B):
    shots = 4096
    x, w = inputs(n, L, B)
    E_exact = qsim(x, w, "cpu")
    E = qsim(x, w, "cpu", shots=shots, seed=SEED, counter=0)
    ratio = (E.double() - E_exact.double()).abs() / shot_bound(E_exact, shots)
    print(f"n={n} L={L} B={B}: max |E_shots - E_exact| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


def test_narrow_host_path_is_unchanged():
    n, B, shots = 12, 3, 257
    p = torch.rand(B, 1 << n, generator=torch.Generator().manual_seed(3))
    p = (p / p.sum(1, keepdim=True)).float().contiguous()
    E, c = sample_z(p, shots, seed=SEED_HI, counter=CTR_HI, return_counts=True)
    Er = torch.empty(B, n)
    cr = torch.empty(B, n, dtype=torch.int32)
    lib = nat.cpu_lib()
    lib.qd_cpu_sample_z.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_uint64] * 2
    lib.qd_cpu_sample_z.restype = ctypes.c_int
    assert lib.qd_cpu_sample_z(p.data_ptr(), Er.data_ptr(), cr.data_ptr(), B, n, shots, SEED_HI, CTR_HI) == 0
    assert torch.equal(E, Er) and torch.equal(c, cr)
    # the narrow entry point keeps its range; the wide one takes over above it
    assert lib.qd_cpu_sample_z(p.data_ptr(), Er.data_ptr(), cr.data_ptr(), 1, 13, shots, 0, 0) == 1


def test_sampler_range():
    with pytest.raises(NotImplementedError, match="16"):
        sample_z(torch.zeros(1, 1 << 17), 8)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_wide_shots_driver_asan_ubsan(tmp_path):
    exe = tmp_path / "qsim_shots_wide_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", os.path.join(CPU, "qsim_cpu.cpp"),
           os.path.join(CPU, "tests", "qsim_shots_wide_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
