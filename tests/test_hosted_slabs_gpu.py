"""The step's gradient slab reductions hosted by conv backward launches (knobs.KNOBS.slabs_hosted; conv.hip
HostedSlabs): extra workgroups of layer 2's fused backward and of layer 1's weight gradient run
slab_rows_sum4_body on slabs that earlier launches completed, so every sum is the slab launch's, bit for bit."""
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as nat
from quantum_distributed_machine_learning_ris_channel_estimation_amd.knobs import KNOBS
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.conv import ConvStackHIP
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.slabsum import SlabBatch
from quantum_distributed_machine_learning_ris_channel_estimation_amd.parallel.dp import DistContext
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.flagship import FlagshipConfig, FlagshipTrainer

pytestmark = pytest.mark.gpu

U = 3


def _model(cuda, pilot_num):
    torch.manual_seed(0)
    a = HDCEModel(pilot_num, cuda, "bf16")
    with torch.no_grad():
        for k in range(3):
            a.bn_w[k].uniform_(0.5, 1.5)
            a.bn_b[k].uniform_(-0.2, 0.2)
    return a


def _grads(a):
    out = {"fc_b": a.fc_b.grad}
    for k in range(3):
        out.update({f"W{k}": a.conv_w[k].grad, f"g{k}": a.bn_w[k].grad, f"b{k}": a.bn_b[k].grad})
    return out


def _conv_backward(cuda, pilot_num, B, accumulate, hosted, first=False):
    """forward + backward of the conv stack with the step's slab batch (an FC-bias job queued first, as the loss pass
    does); returns the gradients the batch's reductions wrote"""
    a = _model(cuda, pilot_num)
    torch.manual_seed(1)
    Yp = torch.randn(3, U, B, 2, a.H, a.W, device=cuda)
    dh = torch.randn(U * B * 3, 32 * a.H * a.W, device=cuda).to(torch.bfloat16)
    colsum = torch.randn(5, a.fc_b.numel(), device=cuda)   # (the FC bias gradient's per-tile column sums)
    conv = ConvStackHIP(a, U, B)
    assert conv.bwd_fused and not conv.bwd_db
    conv.host_slabs, conv.host_first = hosted, first
    conv.forward(a.pack_input(Yp).contiguous(), training=True)
    a.space.zero_grad()
    for g in _grads(a).values():   # accumulate: onto these values; overwrite: they must all disappear
        g.copy_(torch.randn_like(g))
    batch = SlabBatch()
    batch.add(colsum, a.fc_b.grad, 1, colsum.shape[0], colsum.shape[1])
    conv.backward(dh, accumulate=accumulate, slabs=batch)
    # hosted: only layer 1's own weight slab is left (the step hands it to the update)
    assert len(batch.jobs) == (1 if hosted else 10)
    batch.launch(accumulate, nat.stream_ptr(cuda))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _grads(a).items()}


_REF = {}


def _ref(cuda, pilot_num, B, accumulate):
    key = (pilot_num, B, accumulate)
    if key not in _REF:
        _REF[key] = _conv_backward(cuda, pilot_num, B, accumulate, hosted=False)
    return _REF[key]


# B = 40: a ragged last chunk of every kernel; B = 16: fewer samples than one forward workgroup's waves take
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pilot_num,B", [(128, 40), (128, 16), (256, 40), (256, 16)])
def test_hosted_slabs_match_slab_launch(cuda, pilot_num, B, accumulate, first):
    ref = _ref(cuda, pilot_num, B, accumulate)
    got = _conv_backward(cuda, pilot_num, B, accumulate, hosted=True, first=first)
    for name in ref:
        assert torch.isfinite(ref[name]).all(), name
        assert torch.equal(got[name], ref[name]), (name, float((got[name] - ref[name]).abs().max()))


def _state(tr):
    return [tr.hdce.space.flat, tr.qspace.flat, tr.hopt.m, tr.hopt.v, tr.qopt.m, tr.qopt.v,
            tr.hdce.fc_shadow] + list(tr.hdce.run_mean) + list(tr.hdce.run_var)


# serial: backward_conv() on its own (layer 1's slab in a launch); indep: layer 1's slab summed by the update
# (both knobs together at batch 32 / 48: tests/test_gather_in_conv_gpu.py)
@pytest.mark.parametrize("mode,batch", [("indep", 32), ("serial", 32)])
def test_step_with_hosted_slabs_matches_slab_launch(cuda, monkeypatch, mode, batch):
    ctx = DistContext(device=cuda)
    base = dict(batch=batch, data_len=800, use_quantumnat=True, qsc_grid_bwd=128, stream_mode=mode,
                hip_graphs=mode != "serial", steps_per_graph=3)
    trs, losses = [], []
    for on in (False, True):
        monkeypatch.setattr(KNOBS, "slabs_hosted", on)
        tr = FlagshipTrainer(FlagshipConfig(**base), ctx)
        assert tr.slabs_hosted == on and tr.hstep.conv.host_slabs == on
        ls = []
        for _ in range(2):
            tr.run(3)
            torch.cuda.synchronize()
            ls.append(torch.cat([tr.hloss.flatten(), tr.qloss.flatten(), tr.hskip.flatten()]).clone())
        trs.append(tr)
        losses.append(torch.stack(ls))
    assert torch.isfinite(losses[0]).all()
    assert torch.equal(losses[0], losses[1]), (losses[0], losses[1])
    for i, (a, b) in enumerate(zip(_state(trs[0]), _state(trs[1]))):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
