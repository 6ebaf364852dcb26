"""The WaveNet vocoder (fpc_wavenet_*) against a plain reference: a few lines of torch.nn.functional on the CPU, dense over the
whole sequence (dilated conv1d, conv_transpose2d), so nothing in it resembles the cached one-column-per-layer kernel.

Bound rule: the plain reference is evaluated in float32 and in float64 (same folded float32 weights); the kernel may deviate
from the float64 result by 4 x the largest float32-vs-float64 deviation of that output (the 4 covers a different but fixed
summation order).  Every check prints `PARITY <case> <kernel deviation> <bound>`.

To keep the bound meaningful the last layer is scaled so that log_std stays in about [-3, 0], the LPC taps so that
sum |a| = 0.9, and a float64 free run of the reference alone must keep |x| < 100 (free_run_reference)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BASE = dict(num_blocks=2, num_layers=3, inp_channels=1, R=16, G=32, S=16, nfeat=20, cout=16)


def fold(sd, name):
    return torch._weight_norm(sd[name + ".weight_v"], sd[name + ".weight_g"], 0)


@functools.lru_cache(maxsize=None)
def weights(**kw):
    """(state_dict with the reference's keys, config) -- random weights, rows of norm about 1"""
    c = dict(BASE, **kw)
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"embedding.weight": 0.5 * rn(256, 64)}

    def plain(name, *shape):
        sd[name + ".weight"] = rn(*shape) / np.sqrt(np.prod(shape[1:]))
        sd[name + ".bias"] = 0.1 * rn(shape[0])

    def normed(name, *shape, gain=1.0, nbias=None):
        sd[name + ".weight_v"] = rn(*shape)
        sd[name + ".weight_g"] = gain * (0.8 + 0.4 * torch.rand(shape[0], *[1] * (len(shape) - 1), generator=g))
        sd[name + ".bias"] = 0.1 * rn(shape[0] if nbias is None else nbias)

    R, G, S, co = c["R"], c["G"], c["S"], c["cout"]
    plain("c_conv.0", co, c["nfeat"] + 64, 3), plain("c_conv.2", co, co, 3), plain("c_fc.0", co, co), plain("c_fc.2", co, co)
    normed("upsample_conv.0", 1, 1, 3, 20, gain=3.0, nbias=1), normed("upsample_conv.2", 1, 1, 3, 32, gain=3.0, nbias=1)
    normed("front_conv.0.conv", R, c["inp_channels"], 32)
    for n in range(c["num_blocks"] * c["num_layers"]):
        p = f"res_blocks.{n}."
        normed(p + "filter_conv.conv", G, R, 2), normed(p + "gate_conv.conv", G, R, 2)
        normed(p + "filter_conv_c", G, co, 1), normed(p + "gate_conv_c", G, co, 1)
        normed(p + "res_conv", R, G, 1), normed(p + "skip_conv", S, G, 1, gain=0.5)
    normed("final_conv.1.conv", S, S, 1), normed("final_conv.3.conv", 2, S, 1, gain=0.3)
    sd["final_conv.3.conv.bias"] = torch.tensor([0.0, -1.5])
    return sd, c


@functools.lru_cache(maxsize=None)
def build(nu=0, **kw):
    """(model on the GPU, state_dict, config)"""
    from fpcodec_amd.wavenet import Wavenet
    sd, c = weights(**kw)
    R, G, S, co = c["R"], c["G"], c["S"], c["cout"]
    m = Wavenet(out_channels=2, num_blocks=c["num_blocks"], num_layers=c["num_layers"], inp_channels=c["inp_channels"],
                residual_channels=R, gate_channels=G, skip_channels=S, kernel_size=2, cin_channels=c["nfeat"] + 64,
                cout_channels=co, upsample_scales=[10, 16], local=False, fat_upsampler=True, nu=nu)
    return m.load_state_dict(sd), sd, c


@functools.lru_cache(maxsize=None)
def inputs(B, T, nfeat, seed=3):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T, 16, generator=g)
    return dict(feat=0.5 * torch.randn(B, nfeat, T, generator=g), periods=torch.randint(0, 256, (B, T, 1), generator=g),
                lpc=0.9 * a / a.abs().sum(-1, keepdim=True), x=0.3 * torch.randn(B, 160 * T, generator=g),
                noise=torch.randn(B, 160 * T, generator=g))


def ref_upsample(sd, feat, periods, dt):
    w = lambda k: sd[k].to(dt)
    x = torch.cat((feat.to(dt), w("embedding.weight")[periods[:, :, 0]].transpose(1, 2)), 1)
    x = torch.tanh(F.conv1d(x, w("c_conv.0.weight"), w("c_conv.0.bias"), padding=1))
    x = torch.tanh(F.conv1d(x, w("c_conv.2.weight"), w("c_conv.2.bias"), padding=1)).transpose(1, 2)
    x = torch.tanh(F.linear(x, w("c_fc.0.weight"), w("c_fc.0.bias")))
    x = torch.tanh(F.linear(x, w("c_fc.2.weight"), w("c_fc.2.bias"))).transpose(1, 2).unsqueeze(1)
    for i, s in ((0, 10), (2, 16)):
        x = F.conv_transpose2d(x, fold(sd, f"upsample_conv.{i}").to(dt), w(f"upsample_conv.{i}.bias"), stride=(1, s),
                               padding=(1, s // 2))
        x = F.leaky_relu(x, 0.4)
    return x.squeeze(1)


def ref_net(sd, c, x, cfeat, lpc, dt):
    """teacher-forced over the whole sequence, lpc (B,N,16) per sample: stats (B,2,N) of sample i given x[..i-1], pred (B,N)"""
    w, wn = (lambda k: sd[k].to(dt)), (lambda k: fold(sd, k).to(dt))
    x, prev = x.to(dt), lambda v: F.pad(v, (1, 0))[:, :-1]
    u = prev(x)                                                  # the net's input at position p is x[p-1]
    hist = F.pad(u, (15, 0)).unfold(1, 16, 1).flip(-1)           # [b,p,j] = x[p-1-j]
    pred = -(lpc.to(dt) * hist).sum(-1)
    inp = u[:, None] if c["inp_channels"] == 1 else torch.stack((u, prev(x - pred), pred), 1)
    h = F.relu(F.conv1d(F.pad(inp, (31, 0)), wn("front_conv.0.conv"), w("front_conv.0.conv.bias")))
    skip = 0
    for n in range(c["num_blocks"] * c["num_layers"]):
        p, d = f"res_blocks.{n}.", 2 ** (n % c["num_layers"])
        conv = lambda k: (F.conv1d(F.pad(h, (d, 0)), wn(p + k + ".conv"), w(p + k + ".conv.bias"), dilation=d)
                          + F.conv1d(cfeat, wn(p + k + "_c"), w(p + k + "_c.bias")))
        z = torch.tanh(conv("filter_conv")) * torch.sigmoid(conv("gate_conv"))
        skip = skip + F.conv1d(z, wn(p + "skip_conv"), w(p + "skip_conv.bias"))
        h = (h + F.conv1d(z, wn(p + "res_conv"), w(p + "res_conv.bias"))) * np.sqrt(0.5)
    o = F.relu(F.conv1d(F.relu(skip), wn("final_conv.1.conv"), w("final_conv.1.conv.bias")))
    return F.conv1d(o, wn("final_conv.3.conv"), w("final_conv.3.conv.bias")), pred


def ref_stats(sd, c, i, x, dt):
    return ref_net(sd, c, x, ref_upsample(sd, i["feat"], i["periods"], dt), i["lpc"].repeat_interleave(160, 1), dt)


def parity(case, got, ref32, ref64):
    dev, bound = float((got.double() - ref64).abs().max()), 4 * float((ref32.double() - ref64).abs().max())
    print(f"PARITY {case} {dev:.3e} {bound:.3e}")
    assert dev <= bound, f"{case}: kernel deviates {dev:.3e} from float64, bound {bound:.3e}"
    return bound


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("nfeat", [20, 36])
@pytest.mark.parametrize("cout", [16, 36])
def test_upsample(T, nfeat, cout):
    m, sd, _ = build(num_blocks=1, num_layers=1, nfeat=nfeat, cout=cout)
    i = inputs(2, T, nfeat)
    got = m.upsample(i["feat"], i["periods"]).cpu()
    parity(f"upsample T={T} nfeat={nfeat} cout={cout}", got, *(ref_upsample(sd, i["feat"], i["periods"], dt)
                                                              for dt in (torch.float32, torch.float64)))


@pytest.mark.parametrize("kw,B,T", [(dict(inp_channels=1), 1, 2), (dict(inp_channels=1), 17, 2), (dict(inp_channels=3), 1, 2),
                                    (dict(inp_channels=3), 17, 2), (dict(R=32, G=48, S=16), 17, 2),
                                    (dict(num_blocks=1, num_layers=10), 2, 4)])
def test_forward(kw, B, T):
    m, sd, c = build(**kw)
    i = inputs(B, T, c["nfeat"])
    got = m.forward_stats(i["x"], i["feat"], i["periods"], i["lpc"]).cpu()
    parity(f"forward {kw} B={B} T={T}", got, *(ref_stats(sd, c, i, i["x"], dt)[0] for dt in (torch.float32, torch.float64)))


@functools.lru_cache(maxsize=None)
def free_run_reference():
    """float64 free run of the plain reference alone: one utterance, per sample a window one longer than the receptive
    field (ref_net shifts x by one inside it)"""
    sd, c = weights()
    i = {k: v[:1] for k, v in inputs(3, 2, c["nfeat"]).items()}
    cf, lpc = ref_upsample(sd, i["feat"], i["periods"], torch.float64), i["lpc"].repeat_interleave(160, 1)
    rf, x = 32 + 2 * 7, torch.zeros(1, 320).double()
    for n in range(320):
        s = max(0, n - rf)
        st, pred = ref_net(sd, c, x[:, s:n + 1], cf[:, :, s:n + 1], lpc[:, s:n + 1], torch.float64)
        x[0, n] = st[0, 0, -1] + st[0, 1, -1].exp() * i["noise"][0, n] + pred[0, -1]
    return x


@pytest.mark.parametrize("inp", [1, 3])
def test_free_run(inp):
    """each sample against its true history: x[i] - pred64[i] - (mean64[i] + exp(ls64[i]) eps[i]) with the float64 reference
    teacher-forced on the kernel's own x, within the stats bound on the mean plus the same bound times exp(ls)|eps| on the
    noise term (a log_std error of d moves that term by exp(ls)|eps| d)."""
    assert float(free_run_reference().abs().max()) < 100
    m, sd, c = build(inp_channels=inp)
    i = inputs(3, 2, c["nfeat"])
    out, x = (v[:, 0].cpu() for v in m.generate_lpc(i["feat"], i["periods"], i["lpc"], noise=i["noise"], return_x=True))
    assert float(x.abs().max()) < 100
    (s32, _), (s64, pred) = (ref_stats(sd, c, i, x, dt) for dt in (torch.float32, torch.float64))
    bound = 4 * float((s32.double() - s64).abs().max())
    spread = s64[:, 1].exp() * i["noise"].abs()
    resid = (x.double() - pred - (s64[:, 0] + s64[:, 1].exp() * i["noise"])).abs()
    tol = bound * (1 + spread)
    print(f"PARITY free_run inp={inp} {float((resid / tol).max()):.3f} 1 (residual / tolerance, stats bound {bound:.3e})")
    assert bool((resid <= tol).all())
    assert torch.equal(out, 0.85 * F.pad(x, (1, 0))[:, :-1] + x)


def test_placement_and_tile_width():
    """utterance 5 of 17 == the same utterance alone, bit for bit; the NU = 16 and NU = 32 instances agree bit for bit"""
    i = inputs(17, 2, BASE["nfeat"])
    one = {k: v[5:6] for k, v in i.items()}
    res = {}
    for nu in (16, 32):
        m = build(nu=nu)[0]
        res[nu] = m.generate_lpc(i["feat"], i["periods"], i["lpc"], noise=i["noise"])
        alone = m.generate_lpc(one["feat"], one["periods"], one["lpc"], noise=one["noise"])
        assert torch.equal(res[nu][5:6], alone)
    assert torch.equal(res[16], res[32])


def test_philox():
    m, sd, c = build()
    i = inputs(17, 2, c["nfeat"])
    run = lambda seeds: m.generate_lpc(i["feat"], i["periods"], i["lpc"], seeds=seeds, return_x=True)[1][:, 0]
    x = run(np.arange(17))
    assert torch.equal(x, run(np.arange(17)))
    assert not torch.equal(x[0], run(np.arange(17) + 100)[0])
    st = m.forward_stats(x, i["feat"], i["periods"], i["lpc"]).double().cpu()
    pred = ref_stats(sd, c, i, x.cpu(), torch.float64)[1]
    eps = (x.double().cpu() - pred - st[:, 0]) / st[:, 1].exp()
    print(f"PARITY philox mean {float(eps.mean()):+.4f} (0 +- 0.05) variance {float(eps.var()):.4f} (1 +- 0.1)")
    assert abs(float(eps.mean())) < 0.05 and abs(float(eps.var()) - 1) < 0.1


GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g13_wavenet.npz")


def test_golden():
    """the reference's own class (make_golden_wavenet.py): its float32 outputs are the float32 side of the bound"""
    assert os.path.exists(GOLDEN), "tests/golden/g13_wavenet.npz is part of the repository"
    from fpcodec_amd.wavenet import Wavenet
    with np.load(GOLDEN) as z:
        g = {k: torch.from_numpy(z[k]) for k in z.files}
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    c = dict(BASE)
    m = Wavenet(out_channels=2, num_blocks=2, num_layers=3, inp_channels=1, residual_channels=16, gate_channels=32,
                skip_channels=16, kernel_size=2, cin_channels=84, cout_channels=16, upsample_scales=[10, 16], local=False,
                fat_upsampler=True).load_state_dict(sd)
    i = dict(feat=g["feat"], periods=g["periods"].long(), lpc=torch.zeros(1, 3, 16))
    cf64 = ref_upsample(sd, i["feat"], i["periods"], torch.float64)
    parity("golden upsample", m.upsample(i["feat"], i["periods"]).cpu(), g["cfeat"], cf64)
    xk = F.pad(g["x"][:, 0, 1:], (0, 1))  # wavenet() reads x[p] at position p and x[0] = 0: forward's x[p-1]
    got = m.forward_stats(xk, i["feat"], i["periods"], i["lpc"]).cpu()
    parity("golden wavenet", got, g["stats"], ref_net(sd, c, xk, cf64, torch.zeros(1, 480, 16), torch.float64)[0])
