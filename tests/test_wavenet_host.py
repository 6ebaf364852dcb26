"""fpc_wavenet's configuration check and workspace size: pure host functions, no device needed."""
import ctypes as C

import pytest

from fpcodec_amd import _lib

GOOD = dict(out_channels=2, num_blocks=2, num_layers=10, inp_channels=1, residual_channels=128, gate_channels=256,
            skip_channels=128, kernel_size=2, cin_channels=100, cout_channels=128, causal=1, local=0, fat_upsampler=1, nu=0)


def create(**kw):
    c = dict(GOOD, **kw)
    cfg = _lib.WavenetConfig(*[c[n] for n, _ in _lib.WavenetConfig._fields_[:10]], (C.c_int * 2)(10, 16), c["causal"],
                             c["local"], c["fat_upsampler"], c["nu"])
    h = C.c_void_p()
    rc = _lib.lib().fpc_wavenet_create(C.byref(cfg), None, C.byref(h))
    return rc, h, _lib.lib().fpc_last_error().decode()


@pytest.mark.parametrize("kw,status,word", [
    (dict(local=1), -1, "local"), (dict(residual_channels=24), -1, "multiple of 16"), (dict(kernel_size=3), -1, "kernel_size"),
    (dict(out_channels=256), -1, "out_channels"), (dict(causal=0), -1, "causal"), (dict(fat_upsampler=0), -1, "fat_upsampler"),
    (dict(inp_channels=2), -1, "inp_channels"), (dict(cin_channels=144), -1, "cin_channels"),
    (dict(gate_channels=528), -4, "exceed"), (dict(num_layers=11), -4, "exceed"),
    (dict(residual_channels=512, cout_channels=512, nu=32), -4, "LDS")])
def test_refusals(kw, status, word):
    rc, h, text = create(**kw)
    assert rc == status and not h.value and word in text


@pytest.mark.parametrize("B,T", [(1, 1), (17, 3), (33, 10)])
def test_workspace_bytes(B, T):
    """4 (Bp cout 160 T + 12 B T cout + Bp R D), Bp = ceil(B/32) 32, D = blocks (2^layers - 1)  (include/fpcodec.h)"""
    rc, h, text = create()
    assert rc == 0, text
    try:
        Bp = (B + 31) // 32 * 32
        want = 4 * (Bp * 128 * 160 * T + 12 * B * T * 128 + Bp * 128 * 2 * 1023)
        assert _lib.lib().fpc_wavenet_workspace_bytes(h, B, T) == want
        assert _lib.lib().fpc_wavenet_workspace_bytes(h, 0, T) < 0
    finally:
        _lib.lib().fpc_wavenet_destroy(h)


@pytest.mark.parametrize("nfeat", [20, 36])
def test_slice_features(nfeat):
    """fpcodec_amd.synthesis.slice_features against the slicing of src/synthesis.py:97-103, :116 restated"""
    import torch
    from fpcodec_amd.synthesis import slice_features
    c = torch.randn(2, 9, 36, generator=torch.Generator().manual_seed(1))
    feat, lpc, periods = slice_features(c.numpy(), nfeat)
    want = c[:, 2:-2, :-16] if nfeat == 20 else c[:, 2:-2, :]
    assert torch.equal(feat, want.transpose(1, 2)) and feat.shape == (2, nfeat, 5)
    assert torch.equal(lpc, c[:, 2:-2, -16:])
    assert torch.equal(periods, (.1 + 50 * c[:, 2:-2, 18:19] + 100).to(torch.int32)) and periods.shape == (2, 5, 1)
