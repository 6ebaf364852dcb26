"""bitstream.pack_batch / unpack_batch at 128 x 300 (the encoder's own symbols, full codebook sizes) against the host route they
replace: idx.cpu() and bitstream.pack / unpack / entropy_pack / entropy_unpack looped over the utterances.  Device calls: mean
of REP launches between two events after WARM warm-up launches; host: mean of 3 passes.  Prints the record kept as
profiles/bitstream_pack.txt."""
import sys, os, tempfile, time
sys.path.insert(0, '.')
import numpy as np, torch, fpcodec_amd
from fpcodec_amd import bitstream
from fpcodec_amd.vq_func import load_codebooks
from fpcodec_amd.wavernn import Wavernn
B, L, WARM, REP = 128, 300, 20, 200
synth = fpcodec_amd.synth
d = tempfile.mkdtemp(); c = synth.codebooks(); p = {}
for k, v in c.items():
    p[k] = os.path.join(d, k + '.npy'); np.save(p[k], v)
cfg = dict(scl_cb_path=p['scl_hi'], cb_path=p['vq_hi'], bl_scl_cb_path=p['scl_lo'], bl_cb_path=p['vq_lo'])
m = Wavernn(20, 384, 128, 18); m.load_state_dict(synth.predictor_state_dict())
f = torch.from_numpy(synth.predictor_features(B, L, utt0=5000)).cuda()
enc = m.encoder(cfg, f, None, 0.09, 0.28, return_indices=True)
idx = enc[7]
sizes = load_codebooks(cfg['cb_path'], cfg['scl_cb_path'], cfg['bl_cb_path'], cfg['bl_scl_cb_path']).sizes
models = bitstream.Models(sizes, enc[6], (float(enc[4].mean()), float(enc[5].mean())))


def device_ms(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REP):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / REP


def host_ms(fn):
    t = time.perf_counter()
    for _ in range(3):
        out = fn()
    return (time.perf_counter() - t) / 3 * 1e3, out


print(f"bitstream at {B} x {L}, sizes {list(sizes)}, on {torch.cuda.get_device_name(0)}; the symbols are the encoder's")
print(f"{'framing':<14}{'call':<8}{'device ms':>11}{'host route ms':>15}{'ratio':>9}   bits/frame")
for name, mod in (("fixed-length", None), ("entropy-coded", models)):
    data, nbits = bitstream.pack_batch(idx, sizes, mod)
    assert torch.equal(bitstream.unpack_batch(data, L, sizes, mod), idx)
    pk = (lambda u: bitstream.entropy_pack(u, mod)) if mod else (lambda u: bitstream.pack(u, sizes))
    un = (lambda by: bitstream.entropy_unpack(by, L, mod)) if mod else (lambda by: bitstream.unpack(by, L, sizes))
    h_pack, ref = host_ms(lambda: [pk(u) for u in idx.cpu().numpy()])
    h_unpack, back = host_ms(lambda: torch.from_numpy(np.stack([un(by) for by, _ in ref])).cuda())
    same = all(n == int(nbits[b]) and bytes(data[b, :len(by)].cpu().numpy()) == by for b, (by, n) in enumerate(ref))
    assert same and torch.equal(back, idx), "device bytes differ from the host coder's"
    d_pack = device_ms(lambda: bitstream.pack_batch(idx, sizes, mod))
    d_unpack = device_ms(lambda: bitstream.unpack_batch(data, L, sizes, mod))
    bpf = float(nbits.sum()) / (B * L)
    print(f"{name:<14}{'pack':<8}{d_pack:>11.4f}{h_pack:>15.1f}{h_pack / d_pack:>9.0f}   {bpf:.2f}")
    print(f"{name:<14}{'unpack':<8}{d_unpack:>11.4f}{h_unpack:>15.1f}{h_unpack / d_unpack:>9.0f}")
print("device ms = one pack_batch / unpack_batch call, python wrapper and output allocation included; bytes and symbols "
      "checked equal to the host coder's before timing")
