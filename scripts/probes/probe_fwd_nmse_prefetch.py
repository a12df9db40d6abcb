#!/usr/bin/env python3
"""The FC forward with the loss in its epilogue, label rows prefetched by the producer waves (gemm.hip NmsePrefetch,
cfg 8), against the pair it replaces: the plain forward (cfg 8) + the one-pass NMSE kernel.  Flagship shape, synthetic
inputs, a label store large enough that the gathered rows come from HBM; each variant alone on the GPU, timed over
replays of a captured graph.

    python scripts/probes/probe_fwd_nmse_prefetch.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.fc import gemm_fwd  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.nmse import StreamNMSE  # noqa: E402
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel  # noqa: E402


def timed(fn, reps, per_graph=20):
    """us per call, from replays of a captured graph of ``per_graph`` calls (a Python launch costs more than these
    kernels run)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(1, reps // per_graph)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (n * per_graph) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    dev = torch.device("cuda")
    E, U, B, N, K, n_store = 3, 3, 256, 2048, 4096, 2000
    M, S = E * U * B, E * U
    torch.manual_seed(0)
    A = torch.randn(M, K, device=dev).bfloat16()
    W = (torch.randn(N, K, device=dev) * K ** -0.5).bfloat16()
    b = (0.1 * torch.randn(N, device=dev)).bfloat16()
    L = torch.randn(S, n_store, N, device=dev)
    P = L + 0.3 * torch.randn_like(L)
    idx = torch.randperm(n_store, device=dev)[:B]
    u = torch.arange(U, device=dev).view(U, 1, 1)
    e = torch.arange(E, device=dev).view(1, 1, E)
    rowoff = ((e * U + u).expand(U, B, E) * n_store + idx.view(1, B, 1)).reshape(-1).to(torch.int32)
    lab, per = L.reshape(-1, N)[rowoff.long()], P.reshape(-1, N)[rowoff.long()]
    rowden = torch.stack([lab.pow(2).sum(1), per.pow(2).sum(1)], 1).contiguous()
    nm = StreamNMSE(HDCEModel.row_stream(E, U, B, dev), S, N)
    nm.rowoff = rowoff
    bg = torch.empty(N, device=dev)
    Y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.slabsum import SlabBatch

    def plain():
        gemm_fwd(A, W, b, out=Y, cfg=8)

    def loss():   # (as in the step: no finish launch, the bias reduction queued elsewhere)
        nm.fused(Y, L, P, bg, (E, U, B), out_dtype=torch.bfloat16, rowden=rowden, bias_slabs=SlabBatch(), defer_loss=True)

    def pair():
        plain()
        loss()

    def fused():
        nm.gemm_fused(A, W, b, L, P, bg, (E, U, B), rowden, bias_slabs=SlabBatch(), defer_loss=True, cfg=8)

    for name, fn in (("plain forward (cfg 8)", plain), ("one-pass NMSE kernel", loss), ("plain forward + NMSE kernel", pair),
                     ("forward with prefetched loss epilogue", fused)):
        print(f"{name:40s} {timed(fn, reps):7.1f} us", flush=True)


if __name__ == "__main__":
    main()
