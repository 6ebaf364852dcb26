"""Times k_wn_decode (the WaveNet vocoder's sample loop) at the reference's configured shape, src/config.py:48-60:
R/G/S 128/256/128, cout 128, 2 x 10 layers, inp_channels 1, T = 10 frames -- at B = 16, 16 x CUs and 32 x CUs, for each
NU instance.  One warm-up launch per shape, then timed launches through fpc_wavenet_last_decode_ms (device events around
the launch).  Also the only baseline there is: the float32 plain reference through PyTorch on the same GPU, re-evaluating
the receptive field for every sample as wavenet.py:154-191 does, 200 samples at B = 1.

    python tools/time_wavenet.py [--out profiles/wavenet_decode.txt] [--reps 3] [--frames 10]

--forward times the teacher-forced pass instead: forward_stats through the sample loop (T = 10) against the time-parallel
k_wnf_* pass with TN = 32 and 64, T = 10 and 300, B = 16 and 256, device events around the whole call.

    python tools/time_wavenet.py --forward [--out profiles/wavenet_forward.txt] [--reps 3]

--backward times Wavenet.loss_backward (forward + Gaussian loss + backward, k_wnb_*) beside forward() of the same tree, for each
backward tile width, at B = 16 and 64, T = 10, and dense float32 PyTorch autograd of the plain network at 16 x 10.

    python tools/time_wavenet.py --backward [--out profiles/wavenet_backward.txt] [--reps 5]

Operations and bytes are computed from the shapes here; the peak is the 157.3 TFLOP/s f32 MFMA figure DESIGN.md quotes."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fpcodec_amd import _lib  # noqa: E402
from fpcodec_amd.wavenet import Wavenet  # noqa: E402

R, G, S, CO, NB, NL, NFEAT = 128, 256, 128, 128, 2, 10, 36
PEAK = 157.3e12


def state_dict(seed=1):
    g = torch.Generator().manual_seed(seed)
    sd = {"embedding.weight": 0.5 * torch.randn(256, 64, generator=g)}

    def layer(name, *shape, normed=True, gain=1.0):
        v = torch.randn(*shape, generator=g)
        if normed:
            sd[name + ".weight_v"] = v
            sd[name + ".weight_g"] = gain * torch.ones(shape[0], *[1] * (len(shape) - 1))
        else:
            sd[name + ".weight"] = v / np.sqrt(np.prod(shape[1:]))
        sd[name + ".bias"] = 0.1 * torch.randn(shape[0], generator=g)

    layer("c_conv.0", CO, NFEAT + 64, 3, normed=False), layer("c_conv.2", CO, CO, 3, normed=False)
    layer("c_fc.0", CO, CO, normed=False), layer("c_fc.2", CO, CO, normed=False)
    layer("upsample_conv.0", 1, 1, 3, 20, gain=3.0), layer("upsample_conv.2", 1, 1, 3, 32, gain=3.0)
    layer("front_conv.0.conv", R, 1, 32)
    for n in range(NB * NL):
        p = f"res_blocks.{n}."
        layer(p + "filter_conv.conv", G, R, 2), layer(p + "gate_conv.conv", G, R, 2)
        layer(p + "filter_conv_c", G, CO, 1), layer(p + "gate_conv_c", G, CO, 1)
        layer(p + "res_conv", R, G, 1), layer(p + "skip_conv", S, G, 1, gain=0.3)
    layer("final_conv.1.conv", S, S, 1), layer("final_conv.3.conv", 2, S, 1, gain=0.3)
    sd["final_conv.3.conv.bias"] = torch.tensor([0.0, -1.5])
    return sd


def model(sd, nu):
    return Wavenet(out_channels=2, num_blocks=NB, num_layers=NL, inp_channels=1, residual_channels=R, gate_channels=G,
                   skip_channels=S, kernel_size=2, cin_channels=NFEAT + 64, cout_channels=CO, upsample_scales=[10, 16],
                   local=False, fat_upsampler=True, nu=nu).load_state_dict(sd)


def naive_loop(sd, c, rf, samples):
    """wavenet.py:154-191 in float32 on c's device: the whole receptive field again for every sample, B = 1; c (1,cout,>=rf)"""
    dev = c.device
    w = {k: v.to(dev) for k, v in sd.items()}
    fold = lambda k: torch._weight_norm(w[k + ".weight_v"], w[k + ".weight_g"], 0)
    wt = {k[:-9]: fold(k[:-9]) for k in w if k.endswith(".weight_v")}
    x = torch.zeros(1, 1, rf + samples, device=dev)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    sync()
    t0 = time.perf_counter()
    with torch.no_grad():
        for i in range(samples):
            cw = c[:, :, :rf]
            h = F.relu(F.conv1d(F.pad(x[:, :, i:i + rf], (31, 0)), wt["front_conv.0.conv"], w["front_conv.0.conv.bias"]))
            skip = 0
            for n in range(NB * NL):
                p, d = f"res_blocks.{n}.", 2 ** (n % NL)
                conv = lambda k: (F.conv1d(F.pad(h, (d, 0)), wt[p + k + ".conv"], w[p + k + ".conv.bias"], dilation=d)
                                  + F.conv1d(cw, wt[p + k + "_c"], w[p + k + "_c.bias"]))
                z = torch.tanh(conv("filter_conv")) * torch.sigmoid(conv("gate_conv"))
                skip = skip + F.conv1d(z, wt[p + "skip_conv"], w[p + "skip_conv.bias"])
                h = (h + F.conv1d(z, wt[p + "res_conv"], w[p + "res_conv.bias"])) * 0.5 ** 0.5
            o = F.conv1d(F.relu(F.conv1d(F.relu(skip), wt["final_conv.1.conv"], w["final_conv.1.conv.bias"])),
                         wt["final_conv.3.conv"], w["final_conv.3.conv.bias"])[0, :, -1]
            x[0, 0, rf + i] = o[0] + o[1].exp() * torch.randn((), device=dev)
            sync()  # wavenet.py:191
    return samples / (time.perf_counter() - t0)


def forward_leg(a, mac):
    """forward_stats teacher-forced: the sample loop (T = 10 only) against the time-parallel pass, each TN instance; device
    events around the whole call (conditioning and input channels included), one warm-up"""
    sd = state_dict()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"Wavenet.forward_stats on {torch.cuda.get_device_name(0)} ({cus} CUs), R/G/S {R}/{G}/{S}, cout {CO}, {NB} x {NL} layers, "
             f"inp_channels 1; {a.reps} timed calls after one warm-up, device events around the call",
             f"MAC per position and utterance {mac}; TN = positions per workgroup of k_wnf_*, automatic choice "
             f"{model(sd, 0).forward_tile()}; 'loop' = the sequential k_wn_decode with xin set",
             "  path      B     T   positions   ms (min / median)     positions/s   TFLOP/s  of f32 MFMA peak   vs loop"]

    def timed(fn):
        ms = []
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(out).all())
        return min(ms[1:]), float(np.median(ms[1:])), out

    models = {tn: model(sd, 0) for tn in (32, 64)}
    for tn, m in models.items():
        m.set_forward_tile(tn)
    for T in (10, 300):
        for B in (16, 256):
            g = torch.Generator().manual_seed(B + T)
            feat, per = torch.randn(B, NFEAT, T, generator=g).cuda(), torch.randint(0, 256, (B, T, 1), generator=g).cuda()
            lpc = torch.randn(B, T, 16, generator=g)
            lpc = (0.9 * lpc / lpc.abs().sum(-1, keepdim=True)).cuda()
            x = (0.3 * torch.randn(B, 160 * T, generator=g)).cuda()
            npos, loop_ms, loop_out = B * 160 * T, None, None
            legs = ([("loop", lambda: models[64].forward_stats(x, feat, per, lpc))] if T == 10 else []) + \
                   [(f"TN={tn}", lambda m=m: m.forward_stats(x, feat, per, lpc, time_parallel=True)) for tn, m in models.items()]
            for name, fn in legs:
                lo, med, out = timed(fn)
                if name == "loop":
                    loop_ms, loop_out = lo, out
                elif loop_out is not None:
                    assert torch.equal(out, loop_out), "time-parallel stats differ from the sample loop's"
                rate = npos / (lo * 1e-3)
                lines.append(f"{name:>6s} {B:6d} {T:5d} {npos:11d} {lo:10.2f} / {med:<10.2f} {rate:13.0f} {2 * mac * rate / 1e12:9.2f} "
                             f"{100 * 2 * mac * rate / PEAK:10.2f} %" + (f"  {loop_ms / lo:10.1f} x" if loop_ms and name != "loop" else ""))
                print(lines[-1], flush=True)
                del out
            for m in models.values():  # the 25 GB of the largest shape are not kept
                m._fws = m._ws = None
    return lines


def torch_step(sd, inp, cf, y):
    """dense float32 autograd of the plain network on the GPU: loss and gradients of every sample-level weight and of cf"""
    w = {k: v.cuda().requires_grad_() for k, v in sd.items() if k.startswith(("front_conv", "res_blocks", "final_conv"))}
    fold = lambda k: torch._weight_norm(w[k + ".weight_v"], w[k + ".weight_g"], 0)
    cf = cf.detach().requires_grad_()

    def step():
        h = F.relu(F.conv1d(F.pad(inp, (31, 0)), fold("front_conv.0.conv"), w["front_conv.0.conv.bias"]))
        skip = 0
        for n in range(NB * NL):
            p, d = f"res_blocks.{n}.", 2 ** (n % NL)
            conv = lambda k: (F.conv1d(F.pad(h, (d, 0)), fold(p + k + ".conv"), w[p + k + ".conv.bias"], dilation=d)
                              + F.conv1d(cf, fold(p + k + "_c"), w[p + k + "_c.bias"]))
            z = torch.tanh(conv("filter_conv")) * torch.sigmoid(conv("gate_conv"))
            skip = skip + F.conv1d(z, fold(p + "skip_conv"), w[p + "skip_conv.bias"])
            h = (h + F.conv1d(z, fold(p + "res_conv"), w[p + "res_conv.bias"])) * 0.5 ** 0.5
        st = F.conv1d(F.relu(F.conv1d(F.relu(skip), fold("final_conv.1.conv"), w["final_conv.1.conv.bias"])),
                      fold("final_conv.3.conv"), w["final_conv.3.conv.bias"])
        mean, ls = st[:, 0, :-1], st[:, 1, :-1].clamp(min=-9)
        loss = (0.5 * (1.8378770664093453 + 2 * ls + (y[:, 1:] - mean) ** 2 * torch.exp(-2 * ls))).mean()
        return torch.autograd.grad(loss, [v for k, v in w.items() if "res_blocks.%d.res_conv" % (NB * NL - 1) not in k] + [cf])[0]
    return step


def backward_leg(a, mac):
    sd = state_dict()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = model(sd, 0)
    lines = [f"Wavenet.loss_backward on {torch.cuda.get_device_name(0)} ({cus} CUs), R/G/S {R}/{G}/{S}, cout {CO}, {NB} x {NL} layers, "
             f"inp_channels 1, T = 10; {a.reps} timed calls after two warm-ups, device events around the whole call",
             f"MAC per position and utterance: forward {mac}, loss_backward counted as 3 x that; forward tile {m.forward_tile()}",
             "  path            B   positions   ms (min / median / max)    TFLOP/s  of f32 MFMA peak   vs forward()"]

    def timed(fn):
        ms = []
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return min(ms[2:]), float(np.median(ms[2:])), max(ms[2:])

    T = 10
    for B in (16, 64):
        g = torch.Generator().manual_seed(B)
        feat, per = torch.randn(B, NFEAT, T, generator=g).cuda(), torch.randint(0, 256, (B, T, 1), generator=g).cuda()
        x, y = (0.3 * torch.randn(B, 1, 160 * T, generator=g)).cuda(), (0.3 * torch.randn(B, 160 * T, generator=g)).cuda()
        npos = B * 160 * T
        legs = [("forward()", 1, lambda: m.forward(x, per, feat))]
        for btn in (32, 16):
            legs.append((f"loss_backward btn={btn}", 3, lambda btn=btn: (m.set_backward_tile(btn), m.loss_backward(x, per, feat, y))))
        if B == 16:
            legs.append(("torch autograd f32", 3, torch_step(sd, x, m.upsample(feat, per), y)))
        fwd = None
        for name, k, fn in legs:
            lo, med, hi = timed(fn)
            fwd = fwd or lo
            fl = 2 * k * mac * npos / (lo * 1e-3)
            lines.append(f"{name:>22s} {B:4d} {npos:9d} {lo:9.2f} / {med:.2f} / {hi:.2f} {fl / 1e12:10.2f} {100 * fl / PEAK:10.2f} % {lo / fwd:12.2f} x")
            print(lines[-1], flush=True)
        m.set_backward_tile(0)
        lines.append(f"  workspace {m.backward_workspace_bytes(B, T) / 1e9:.2f} GB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/wavenet_decode.txt, with --forward profiles/wavenet_forward.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--forward", action="store_true", help="time the teacher-forced pass instead of the sample loop")
    ap.add_argument("--backward", action="store_true", help="time loss_backward beside forward() and torch autograd")
    a = ap.parse_args()
    a.out = a.out or ("profiles/wavenet_backward.txt" if a.backward else "profiles/wavenet_forward.txt" if a.forward
                      else "profiles/wavenet_decode.txt")
    _lib.require_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T, N, L = a.frames, a.frames * 160, NB * NL
    mac = R * 32 + L * (2 * G * (2 * R + CO) + (R + S) * G) - R * G + S * S + 2 * S
    if a.forward or a.backward:
        lines = backward_leg(a, mac) if a.backward else forward_leg(a, mac)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    wbytes = 4 * (R * 32 + L * (2 * G * (2 * R + CO) + (R + S) * G) - R * G + S * S + 16 * S)
    sd = state_dict()
    lines = [f"k_wn_decode on {torch.cuda.get_device_name(0)} ({cus} CUs), R/G/S {R}/{G}/{S}, cout {CO}, {NB} x {NL} layers, "
             f"inp_channels 1, T = {T} frames ({N} samples); {a.reps} timed launches after one warm-up, device events",
             f"MAC per sample and utterance {mac}; weights streamed per sample step and workgroup {wbytes} bytes",
             "   NU      B  tiles   ms (min / median)  us/step   samples/s  per stream   TFLOP/s  of f32 MFMA peak"]
    for nu in (16, 32):
        m = model(sd, nu)
        for B in (16, 16 * cus, 32 * cus):
            g = torch.Generator().manual_seed(B)
            feat, per = torch.randn(B, NFEAT, T, generator=g), torch.randint(0, 256, (B, T, 1), generator=g)
            lpc = torch.randn(B, T, 16, generator=g)
            lpc = (0.9 * lpc / lpc.abs().sum(-1, keepdim=True)).cuda()
            feat, per = feat.cuda(), per.cuda()
            ms = []
            for r in range(a.reps + 1):
                out = m.generate_lpc(feat, per, lpc, seeds=np.arange(B))
                ms.append(m.last_decode_ms())
            assert bool(torch.isfinite(out).all())
            lo, med = min(ms[1:]), float(np.median(ms[1:]))
            rate = B * N / (lo * 1e-3)
            lines.append(f"{nu:5d} {B:6d} {(B + nu - 1) // nu:6d} {lo:10.2f} / {med:<8.2f} {lo * 1e3 / N:8.1f} {rate:11.0f} "
                         f"{rate / B:11.1f} {2 * mac * rate / 1e12:9.2f} {100 * 2 * mac * rate / PEAK:10.2f} %")
            print(lines[-1], flush=True)
            del out, feat, per, lpc
        base_model = m
    rf = base_model.receptive_field_size()
    frames = -(-rf // 160)
    c = base_model.upsample(torch.randn(1, NFEAT, frames), torch.randint(0, 256, (1, frames, 1)))
    lines.append(f"reference-style loop (float32 torch on the same GPU, receptive field {rf} re-evaluated per sample, B = 1, "
                 f"200 samples): {naive_loop(sd, c, rf, 200):.1f} samples/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
