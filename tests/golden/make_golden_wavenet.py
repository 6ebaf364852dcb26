"""Golden vectors of the reference's own vocoder, Wavenet (src/models/wavenet.py), SURVEY row 13.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_wavenet.py
Writes tests/golden/g13_wavenet.npz: the state_dict of a small model ("sd." + the reference's key), inputs for 3 frames,
upsample()'s output and wavenet()'s (mean, log_std) over a fixed 480-sample x.  Arrays and key names only.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    loss = types.ModuleType("loss")
    loss.gaussian_loss = loss.KL_gaussians = None
    sys.modules["tqdm"], sys.modules["loss"] = tq, loss
    sys.path.insert(0, "/root/reference/src/models")       # wavenet.py says `from modules import`
    from models.wavenet import Wavenet
    torch.manual_seed(20221113)
    m = Wavenet(out_channels=2, num_blocks=2, num_layers=3, inp_channels=1, residual_channels=16, gate_channels=32,
                skip_channels=16, kernel_size=2, cin_channels=20 + 64, cout_channels=16, upsample_scales=[10, 16],
                local=False, fat_upsampler=True).eval()
    with torch.no_grad():
        # keep log_std in about [-3, 0] (tests/test_gpu_wavenet.py): a small last layer around a bias of -1.5
        m.final_conv[3].conv.weight_g.mul_(0.3)
        m.final_conv[3].conv.bias.copy_(torch.tensor([0.0, -1.5]))
        feat = 0.5 * torch.randn(1, 20, 3)
        periods = torch.randint(0, 256, (1, 3, 1))
        x = 0.3 * torch.randn(1, 1, 480)
        x[:, :, 0] = 0.0
        cfeat = m.upsample(feat, periods)
        stats = m.wavenet(x, cfeat)
    out = {"sd." + k: v.numpy() for k, v in m.state_dict().items()}
    out.update(feat=feat.numpy(), periods=periods.numpy().astype(np.int32), x=x.numpy(), cfeat=cfeat.numpy(),
               stats=stats.numpy())
    path = os.path.join(HERE, "g13_wavenet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
