"""The time-parallel teacher-forced pass of the WaveNet vocoder (k_wnf_*, csrc/wavenet_forward.h) against the plain float64
reference and bound rule of test_gpu_wavenet.py, and bit for bit against the sequential sample loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_wavenet as wn

pytestmark = pytest.mark.gpu
CONFIGURED = dict(R=128, G=256, S=128, cout=128, num_blocks=2, num_layers=10)


def refs(sd, c, i):
    return [wn.ref_stats(sd, c, i, i["x"], dt)[0] for dt in (torch.float32, torch.float64)]


@pytest.mark.parametrize("kw,B,T", [(dict(inp_channels=1), 1, 1), (dict(inp_channels=1), 17, 2), (dict(inp_channels=3), 1, 1),
                                    (dict(inp_channels=3), 17, 2), (dict(R=32, G=48, S=16, cout=36), 3, 2),
                                    (dict(num_blocks=1, num_layers=10), 2, 4), (CONFIGURED, 2, 7)])
def test_forward_time_parallel(kw, B, T):
    m, sd, c = wn.build(**kw)
    i = wn.inputs(B, T, c["nfeat"])
    got = m.forward_stats(i["x"], i["feat"], i["periods"], i["lpc"], time_parallel=True).cpu()
    wn.parity(f"forward_parallel {kw} B={B} T={T} tn={m.forward_tile()}", got, *refs(sd, c, i))
    assert torch.equal(got, m.forward_stats(i["x"], i["feat"], i["periods"], i["lpc"], time_parallel=False).cpu())
    if kw is CONFIGURED:  # also the instance that fills the LDS at these widths (160 KiB), which the host does not pick
        m.set_forward_tile(64)
        try:
            wide = m.forward_stats(i["x"], i["feat"], i["periods"], i["lpc"], time_parallel=True).cpu()
        finally:
            m.set_forward_tile(0)
        assert torch.equal(got, wide)


def test_tile_width_and_placement():
    """every TN instance gives the same bits; utterance 5 of 17 == the same utterance alone"""
    from fpcodec_amd.wavenet import Wavenet
    sd, c = wn.weights()
    i = wn.inputs(17, 2, c["nfeat"])
    one = {k: v[5:6] for k, v in i.items()}
    res = {}
    for tn in (16, 32, 64):
        m = Wavenet(out_channels=2, num_blocks=c["num_blocks"], num_layers=c["num_layers"], inp_channels=1,
                    residual_channels=c["R"], gate_channels=c["G"], skip_channels=c["S"], kernel_size=2,
                    cin_channels=c["nfeat"] + 64, cout_channels=c["cout"], upsample_scales=[10, 16], local=False,
                    tn=tn).load_state_dict(sd)
        assert m.forward_tile() == tn
        res[tn] = m.forward_stats(i["x"], i["feat"], i["periods"], i["lpc"], time_parallel=True)
        alone = m.forward_stats(one["x"], one["feat"], one["periods"], one["lpc"], time_parallel=True)
        assert torch.equal(res[tn][5:6], alone)
    assert torch.equal(res[32], res[64]) and torch.equal(res[16], res[64])


@pytest.mark.parametrize("inp", [1, 3])
def test_reference_forward_signature(inp):
    """forward(x, periods, c) on input channels built on the CPU in float32 as ref_net builds them"""
    m, sd, c = wn.build(inp_channels=inp)
    B, T = 3, 2
    i = wn.inputs(B, T, c["nfeat"])
    prev = lambda v: F.pad(v, (1, 0))[:, :-1]
    u = prev(i["x"])
    hist = F.pad(u, (15, 0)).unfold(1, 16, 1).flip(-1)
    pred = -(i["lpc"].repeat_interleave(160, 1) * hist).sum(-1)
    x = u[:, None] if inp == 1 else torch.stack((u, prev(i["x"] - pred), pred), 1)
    got = m.forward(x, i["periods"], i["feat"]).cpu()
    assert got.shape == (B, 2, 160 * T) and m(x, i["periods"], i["feat"]).shape == got.shape
    wn.parity(f"forward(x, periods, c) inp={inp}", got, *refs(sd, c, i))


def test_golden_forward():
    """golden G13: the reference's own class through the reference's own signature; its x is already the net's input"""
    from fpcodec_amd.wavenet import Wavenet
    with np.load(wn.GOLDEN) as z:
        g = {k: torch.from_numpy(z[k]) for k in z.files}
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    m = Wavenet(out_channels=2, num_blocks=2, num_layers=3, inp_channels=1, residual_channels=16, gate_channels=32,
                skip_channels=16, kernel_size=2, cin_channels=84, cout_channels=16, upsample_scales=[10, 16], local=False,
                fat_upsampler=True).load_state_dict(sd)
    got = m.forward(g["x"], g["periods"].long(), g["feat"]).cpu()
    cf64 = wn.ref_upsample(sd, g["feat"], g["periods"].long(), torch.float64)
    xk = F.pad(g["x"][:, 0, 1:], (0, 1))  # ref_net shifts by one itself
    wn.parity("golden forward", got, g["stats"], wn.ref_net(sd, dict(wn.BASE), xk, cf64, torch.zeros(1, 480, 16), torch.float64)[0])
