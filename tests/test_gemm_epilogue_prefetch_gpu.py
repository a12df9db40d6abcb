"""The FC forward whose producer waves prefetch the loss epilogue's label rows (csrc/hip/gemm.hip NmsePrefetch, tile
configuration 8) against the pair of launches it replaces -- the plain forward (bias epilogue, bf16 Y) + the one-pass
NMSE kernel (csrc/hip/nmse.hip) -- on identical inputs: dY and the bias gradient's partial rows bit-identical, the
loss scalars equal up to fp32 summation order, and one flagship step leaving bit-identical HDCE parameters."""
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.knobs import KNOBS
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.fc import gemm_fwd, gemm_fwd_ok

pytestmark = pytest.mark.gpu

CFG = 8        # the producer-wave forward tile (144 x 128, 4-stage ring)
RTOL = 2e-3    # tests/test_gemm_gpu.py::test_gemm_nmse_epilogue_matches_fp32's loss tolerance


def _problem(E, U, B, N, K, device, n_store=40):
    """Inputs of the loss epilogue: a label / perfect-channel store, random row offsets WITH repeated rows (every
    stream draws the same B of n_store samples), per-row powers."""
    torch.manual_seed(3)
    M, S = E * U * B, E * U
    A = torch.randn(M, K, device=device).bfloat16()
    W = (torch.randn(N, K, device=device) * K ** -0.5).bfloat16()
    b = (0.1 * torch.randn(N, device=device)).bfloat16()
    L = torch.randn(S, n_store, N, device=device)
    P = L + 0.3 * torch.randn_like(L)
    idx = torch.randint(0, n_store, (B,), device=device)
    u = torch.arange(U, device=device).view(U, 1, 1)
    e = torch.arange(E, device=device).view(1, 1, E)
    rowoff = ((e * U + u).expand(U, B, E) * n_store + idx.view(1, B, 1)).reshape(-1).to(torch.int32)
    lab = L.reshape(-1, N)[rowoff.long()]
    per = P.reshape(-1, N)[rowoff.long()]
    rowden = torch.stack([lab.pow(2).sum(1), per.pow(2).sum(1)], 1).contiguous()
    return A, W, b, L, P, rowoff, rowden


def _two_kernel(A, W, b, L, P, rowoff, rowden, E, U, B):
    """Plain forward + one-pass NMSE kernel.  That kernel walks 1024 columns per block: a narrower problem runs
    zero-padded to 1024 columns (Y, label and perf all zero there: the extra columns add exact zeros to the error
    sums, and every real column's dY and partial sums are computed exactly as in a 1024-column problem)."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.nmse import StreamNMSE
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel
    M, N = A.shape[0], W.shape[0]
    S = E * U
    Y = gemm_fwd(A, W, b, cfg=CFG)
    Np = -(-N // 1024) * 1024
    if Np != N:
        Yp = torch.zeros(M, Np, device=A.device, dtype=Y.dtype)
        Yp[:, :N] = Y
        Lp, Pp = (torch.zeros(S, t.shape[1], Np, device=A.device) for t in (L, P))
        Lp[..., :N], Pp[..., :N] = L, P
        Y, L, P = Yp, Lp, Pp
    nm = StreamNMSE(HDCEModel.row_stream(E, U, B, A.device), S, Np)
    nm.rowoff = rowoff
    bg = torch.full((Np,), 1e30, device=A.device)
    dY = nm.fused(Y, L, P, bg, (E, U, B), out_dtype=torch.bfloat16, rowden=rowden)
    torch.cuda.synchronize()
    colsum = nm._fz[1]
    return dY[:, :N].clone(), colsum[:, :N].clone(), bg[:N].clone(), nm.loss.clone(), float(nm.skip)


# M = 576: 4 row tiles of 144 that straddle the user groups (B E = 192), 2 column tiles.  K = 320: 5 K steps, one more
# than the ring depth -- two steady-state steps carry prefetch loads, the rest is issued after the loop; K = 64, the
# smallest the launcher accepts: no steady-state step at all; K = 4096: more steps than the prefetch is spread over.
@pytest.mark.parametrize("E,U,B,N,K", [(3, 3, 64, 256, 320), (3, 3, 64, 256, 64), (3, 3, 64, 256, 4096)])
def test_prefetched_loss_forward_matches_two_kernel_path(cuda, E, U, B, N, K):
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.nmse import StreamNMSE
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel
    M, S = E * U * B, E * U
    assert gemm_fwd_ok(M, N, K, CFG)
    A, W, b, L, P, rowoff, rowden = _problem(E, U, B, N, K, cuda)
    ref_dY, ref_colsum, ref_bg, ref_loss, ref_skip = _two_kernel(A, W, b, L, P, rowoff, rowden, E, U, B)
    nm = StreamNMSE(HDCEModel.row_stream(E, U, B, cuda), S, N)
    nm.rowoff = rowoff
    bg = torch.full((N,), 1e30, device=cuda)
    dY = nm.gemm_fused(A, W, b, L, P, bg, (E, U, B), rowden, cfg=CFG)
    torch.cuda.synchronize()
    colsum = nm._gz[3]
    print("loss", nm.loss.tolist(), "two-kernel", ref_loss.tolist(),
          "dY mismatches", int((dY.view(torch.int16) != ref_dY.view(torch.int16)).sum()),
          "colsum mismatches", int((colsum != ref_colsum).sum()))
    assert torch.equal(dY.view(torch.int16), ref_dY.view(torch.int16))
    assert colsum.shape == ref_colsum.shape and torch.equal(colsum, ref_colsum)
    assert torch.equal(bg, ref_bg)
    assert torch.allclose(nm.loss, ref_loss, rtol=RTOL), (nm.loss, ref_loss)
    assert float(nm.skip) == 0.0 and ref_skip == 0.0
    # a row the swapped-row check can see: dY of a row depends on ITS label row
    lab = L.reshape(-1, N)[rowoff.long()]
    den = torch.zeros(S, device=cuda).index_add_(0, HDCEModel.row_stream(E, U, B, cuda).long(), lab.pow(2).sum(1))
    Y = gemm_fwd(A, W, b, cfg=CFG).float()
    want = (2.0 / (S * den))[HDCEModel.row_stream(E, U, B, cuda).long()][:, None] * (Y - lab)
    assert float((dY.float() - want).abs().max()) <= 1e-2 * float(want.abs().max())
    A[3, 3] = float("nan")
    nm.gemm_fused(A, W, b, L, P, bg, (E, U, B), rowden, cfg=CFG)
    torch.cuda.synchronize()
    assert float(nm.skip) == 1.0


def test_prefetched_loss_forward_without_perfect_channel(cuda):
    """perf = None: the producers' load count stays fixed (the label rows again), the values unused."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.nmse import StreamNMSE
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel
    E, U, B, N, K = 3, 3, 64, 256, 320
    A, W, b, L, P, rowoff, rowden = _problem(E, U, B, N, K, cuda)
    outs = []
    for perf in (P, None):
        nm = StreamNMSE(HDCEModel.row_stream(E, U, B, cuda), E * U, N)
        nm.rowoff = rowoff
        bg = torch.full((N,), 1e30, device=cuda)
        dY = nm.gemm_fused(A, W, b, L, perf, bg, (E, U, B), rowden, cfg=CFG)
        torch.cuda.synchronize()
        outs.append((dY.clone(), bg, nm.loss.clone()))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][2][0]) == float(outs[1][2][0])


@pytest.mark.parametrize("mode", ["serial", "indep"])
def test_flagship_step_fused_forward_matches_plain_forward(cuda, monkeypatch, mode):
    """One flagship step with the loss in the forward's epilogue (KNOBS.hand_gemm "fwd") against the plain forward +
    the NMSE kernel ("fwdplain"): every HDCE parameter bit-identical after the update."""
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.parallel.dp import DistContext
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.flagship import (FlagshipConfig,
                                                                                                FlagshipTrainer)
    ctx = DistContext(device=cuda)
    trs = []
    for hg, path in (("fwd,wgrad,dgrad", "hand"), ("fwdplain,wgrad,dgrad", "hand_plain")):
        monkeypatch.setattr(KNOBS, "hand_gemm", hg)
        torch.manual_seed(0)
        tr = FlagshipTrainer(FlagshipConfig(batch=64, data_len=800, hip_graphs=False, stream_mode=mode), ctx)
        tr.step()
        torch.cuda.synchronize()
        assert tr.hstep.fc_path == path
        trs.append(tr)
    a, b = trs
    print("hloss", a.hloss.tolist(), b.hloss.tolist())
    sp = a.hdce.space
    for name, p in zip(sp.names, sp.params):
        sl = sp.slice_of(p)
        assert torch.equal(a.hdce.space.flat[sl], b.hdce.space.flat[sl]), name
    assert torch.equal(a.hdce.fc_shadow, b.hdce.fc_shadow)
    assert torch.allclose(a.hloss, b.hloss, rtol=RTOL), (a.hloss, b.hloss)
    assert float(a.skip_flags().sum()) == 0.0
