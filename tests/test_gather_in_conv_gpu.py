"""The HDCE chain's batch gather inside the conv layer-1 kernels (knobs.KNOBS.gather_in_conv; conv.hip GatherSrc /
RowSrc): the forward reads the pilots from the HBM store and writes rowoff / rowden, the weight gradient re-reads
them through rowoff.  Only WHERE the same values are read changes, so everything is compared with torch.equal."""
import pytest
import torch

from quantum_distributed_machine_learning_ris_channel_estimation_amd.data.datasets import make_dml_stores
from quantum_distributed_machine_learning_ris_channel_estimation_amd.knobs import KNOBS
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.conv import ConvStackHIP
from quantum_distributed_machine_learning_ris_channel_estimation_amd.ops.gather import StepGather
from quantum_distributed_machine_learning_ris_channel_estimation_amd.parallel.dp import DistContext
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.engine import HDCEModel
from quantum_distributed_machine_learning_ris_channel_estimation_amd.train.flagship import FlagshipConfig, FlagshipTrainer

pytestmark = pytest.mark.gpu

U = 3
_STORE = {}


def _store(cuda, pilot_num):
    """a store of 270 rows per stream, its row powers and a permutation (shared, read-only)"""
    if pilot_num not in _STORE:
        st, _ = make_dml_stores(300, pilot_num, 10, 0.9, "cpu", synthetic=True, base_seed=5)
        d = st.to(cuda)
        rp = (d.Hlabel.pow(2).sum(-1).reshape(-1).contiguous(), d.Hperf.pow(2).sum(-1).reshape(-1).contiguous())
        torch.manual_seed(2)
        _STORE[pilot_num] = (d, rp, torch.randperm(d.n, device=cuda))
    return _STORE[pilot_num]


def _run(cuda, pilot_num, B, cursor, in_conv):
    d, rp, perm = _store(cuda, pilot_num)
    torch.manual_seed(0)
    a = HDCEModel(pilot_num, cuda, "bf16")
    with torch.no_grad():
        for k in range(3):
            a.bn_w[k].uniform_(0.5, 1.5)
            a.bn_b[k].uniform_(-0.2, 0.2)
    g = StepGather(3, U, B, a.H, a.W, cuda, with_classifier=False)
    g.rowpow = rp
    cur = torch.full((1,), cursor, dtype=torch.int32, device=cuda)
    conv = ConvStackHIP(a, U, B, spw=KNOBS.conv_spw)
    if in_conv:
        g.x1.fill_(float("nan"))      # (never read)
        g.rowoff.fill_(-1)
        g.in_conv(d, perm, cur)
    else:
        g.from_cursor(d, perm, cur, None, hdce=True, classifier=False)
    conv.gather_src = g.fused
    assert (g.fused is not None) == in_conv
    h3 = conv.forward(g.x1, training=True)
    torch.manual_seed(1)
    dh = torch.randn(U * B * 3, 32 * a.H * a.W, device=cuda).to(torch.bfloat16)
    a.space.zero_grad()
    conv.backward(dh, accumulate=False)
    torch.cuda.synchronize()
    assert int(cur) == cursor   # (read only)
    return dict(z0=conv.z[0].clone(), stats0=conv.stats[0].clone(), rowoff=g.rowoff.clone(), rowden=g.rowden.clone(),
                h3=h3.clone(), wslab0=conv.wslab[0].clone(), dW0=a.conv_w[0].grad.clone(),
                dW1=a.conv_w[1].grad.clone())


# B = 40: the last chunk of 4 * conv_spw = 12 samples is ragged; B = 16: fewer samples than a workgroup's waves take.
# cursor 0, a non-zero one, and one with c + B > nperm (270 rows), where the guard picks 0
@pytest.mark.parametrize("cursor", [0, 57, 260])
@pytest.mark.parametrize("pilot_num,B", [(128, 40), (128, 16), (256, 40), (256, 16)])
def test_gather_in_conv_forward_backward(cuda, pilot_num, B, cursor):
    ref = _run(cuda, pilot_num, B, cursor, in_conv=False)
    got = _run(cuda, pilot_num, B, cursor, in_conv=True)
    assert torch.isfinite(ref["z0"].float()).all() and torch.isfinite(ref["dW0"]).all()
    for name in ref:
        assert torch.equal(got[name], ref[name]), name
    if cursor == 260:   # the guarded cursor reads the permutation's head
        d, _, perm = _store(cuda, pilot_num)
        lsr = d.Hlabel.stride(0) // d.Hlabel.shape[-1]
        assert torch.equal(got["rowoff"].view(U, B, 3)[0, :, 0].long() % lsr, perm[:B])


def _state(tr):
    return [tr.hdce.space.flat, tr.qspace.flat, tr.hopt.m, tr.hopt.v, tr.qopt.m, tr.qopt.v,
            tr.hdce.fc_shadow] + list(tr.hdce.run_mean) + list(tr.hdce.run_var)


# batch 48: a size the loss epilogue does not tile
@pytest.mark.parametrize("batch", [32, 48])
def test_step_with_both_fusions_matches_plain_chain(cuda, monkeypatch, batch):
    """6 graphed steps of the world-1 indep plan with gather_in_conv and slabs_hosted on == both off: losses, NaN
    flags and every HDCE / QSC parameter, optimizer moment and BN statistic."""
    ctx = DistContext(device=cuda)
    base = dict(batch=batch, data_len=800, use_quantumnat=True, qsc_grid_bwd=128, stream_mode="indep",
                hip_graphs=True, steps_per_graph=3)
    trs, losses = [], []
    for on in (False, True):
        monkeypatch.setattr(KNOBS, "slabs_hosted", on)
        monkeypatch.setattr(KNOBS, "gather_in_conv", on)
        tr = FlagshipTrainer(FlagshipConfig(**base), ctx)
        assert tr.slabs_hosted == on and tr.gather_in_conv == on
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
