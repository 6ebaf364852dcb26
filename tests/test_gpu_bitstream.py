"""Device-side bitstream (fpc_bitstream_pack / _unpack) against its specification, the pure-Python coders of
fpcodec_amd/bitstream.py: the same bytes, the same bit counts, the same symbols back.  All comparisons are exact."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = {"full": [256, 16, 1024, 1024, 256], "hi": [256, 0, 1024, 1024, 0], "one": [256, 0, 256, 0, 0],
         "zero": [1, 0, 2, 0, 0], "wide": [2048, 0, 4096, 4096, 0]}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from fpcodec_amd import _lib
    _lib.require_gpu()
    return torch


def draw(sizes, B, L, seed, models):
    """valid symbols with flag rates of 0.3, and (models=True) field models from histograms with some zero counts"""
    from fpcodec_amd import bitstream
    rng = np.random.default_rng(seed)
    n_hi, n_lo, N0, N1, Nl = sizes
    i1, i2 = rng.random((B, L)) < 0.3, rng.random((B, L)) < 0.3
    x = np.full((B, L, 4), -1, np.int32)
    x[..., 0] = np.where(i1, rng.integers(0, n_hi, (B, L)), n_hi + rng.integers(0, n_lo, (B, L)) if n_lo else -1)
    x[..., 1] = np.where(i2, rng.integers(0, N0, (B, L)), -1)
    if N1:
        x[..., 2] = np.where(i2, rng.integers(0, N1, (B, L)), -1)
    if Nl:
        x[..., 3] = np.where(i2, -1, rng.integers(0, Nl, (B, L)))
    hist = [rng.integers(1, 50, n) * (rng.random(n) < 0.8) for n in sizes]
    return x, bitstream.Models(sizes, hist, (0.3, 0.3)) if models else None


def reference(x, sizes, models):
    from fpcodec_amd import bitstream
    return [bitstream.entropy_pack(u, models) if models else bitstream.pack(u, sizes) for u in x]


def check_against_reference(x, sizes, models):
    from fpcodec_amd import bitstream
    B, L = x.shape[:2]
    data, nbits = bitstream.pack_batch(x, sizes, models)
    assert data.shape[1] == bitstream.bound(sizes, L, models is not None)
    got, nbits = data.cpu().numpy(), nbits.cpu().numpy()
    ref = reference(x, sizes, models)
    theirs = np.zeros((B, max(len(by) for by, _ in ref)), np.uint8)
    for b, (by, n) in enumerate(ref):
        assert nbits[b] == n <= 8 * got.shape[1], (b, nbits[b], n)
        assert np.array_equal(got[b, :len(by)], np.frombuffer(by, np.uint8)), b
        assert not got[b, len(by):].any(), b
        theirs[b, :len(by)] = np.frombuffer(by, np.uint8)
    assert np.array_equal(bitstream.unpack_batch(data, L, sizes, models).cpu().numpy(), x)
    assert np.array_equal(bitstream.unpack_batch(theirs, L, sizes, models).cpu().numpy(), x)  # cross-decodable
    return ref


@pytest.mark.parametrize("entropy", [False, True])
@pytest.mark.parametrize("which,B,L", [("full", 5, 300), ("full", 65, 40), ("hi", 3, 63), ("hi", 2, 65), ("one", 1, 1),
                                       ("one", 65, 40), ("zero", 3, 63), ("wide", 2, 65)])
def test_both_framings_match_the_reference(torch_cuda, which, B, L, entropy):
    x, models = draw(SIZES[which], B, L, 1000 * B + L, entropy)
    check_against_reference(x, SIZES[which], models)


@pytest.fixture(scope="module")
def pending_run():
    """300 frames that keep the coder's interval astride _HALF: every field takes the symbol whose sub-interval holds
    _HALF, so nearly every renormalisation is an underflow step and one pending run spans the utterance"""
    from fpcodec_amd import bitstream as bs
    sizes = SIZES["hi"]
    models = bs.Models(sizes, [np.ones(n) for n in sizes], (1.0, 1.0))
    x = np.full((1, 300, 4), -1, np.int32)
    low, high = 0, bs._TOP
    for i in range(300):
        for col, name in ((None, "f1"), (None, "f2"), (0, "scl_hi"), (1, "v0"), (2, "v1")):
            m, rng, sym = getattr(models, name), high - low + 1, 1  # both flags set
            if col is not None:
                sym = int(np.searchsorted(m.cum, ((bs._HALF - low + 1) * m.total - 1) // rng, side="right")) - 1
                x[0, i, col] = sym
            low, high = low + rng * int(m.cum[sym]) // m.total, low + rng * int(m.cum[sym + 1]) // m.total - 1
            while True:
                if high < bs._HALF or low >= bs._HALF:
                    low, high = low & (bs._HALF - 1), high & (bs._HALF - 1)
                elif low >= bs._QTR and high < bs._HALF + bs._QTR:
                    low, high = low - bs._QTR, high - bs._QTR
                else:
                    break
                low, high = low << 1, (high << 1) | 1
    return x, sizes, models


def test_long_pending_run(torch_cuda, pending_run):
    x, sizes, models = pending_run
    (by, n), = check_against_reference(x, sizes, models)
    bits = np.unpackbits(np.frombuffer(by, np.uint8))[:n]
    runs = np.diff(np.flatnonzero(np.concatenate([[1], np.diff(bits), [1]])))
    assert n > 8000 and runs.max() > 8000, (n, runs.max())  # the input does what it is for


@pytest.mark.parametrize("entropy", [False, True])
def test_truncation_and_guard_bytes(torch_cuda, pending_run, entropy):
    torch = torch_cuda
    from fpcodec_amd import _lib, bitstream
    if entropy:
        x, sizes, models = pending_run
    else:
        sizes = SIZES["wide"]
        x, models = draw(sizes, 3, 65, 7, False)
    B, L = x.shape[:2]
    ref = reference(x, sizes, models)
    stride = max(len(by) for by, _ in ref) // 2
    buf = torch.full((B * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    nbits, nbits0 = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    idx, h = torch.from_numpy(x).cuda(), models.device_handle() if models else None
    for data, pitch, out in ((buf.data_ptr(), stride, nbits), (None, 0, nbits0)):
        _lib.check(_lib.lib().fpc_bitstream_pack(bitstream._sizes_arg(sizes), h, idx.data_ptr(), B, L, data, pitch,
                                                 out.data_ptr(), _lib.stream_ptr()), "fpc_bitstream_pack")
    got = buf.cpu().numpy()
    assert (got[B * stride:] == 0xA5).all()
    for b, (by, n) in enumerate(ref):
        assert nbits[b] == nbits0[b] == n > 8 * stride
        assert np.array_equal(got[b * stride:(b + 1) * stride], np.frombuffer(by, np.uint8)[:stride]), b


@pytest.mark.parametrize("entropy", [False, True])
def test_invalid_symbols_are_refused_per_utterance(torch_cuda, entropy):
    from fpcodec_amd import bitstream
    sizes = SIZES["full"]
    x, models = draw(sizes, 4, 70, 11, entropy)
    ref = reference(x, sizes, models)
    x[1, 66] = (3, 1024, 0, -1)   # stage-1 index >= its table size
    x[2, 5] = (-1, 7, 7, -1)      # the below-threshold scalar book exists, its symbol is missing
    data, nbits = bitstream.pack_batch(x, sizes, models)
    got, nbits = data.cpu().numpy(), nbits.cpu().numpy()
    assert list(nbits) == [ref[0][1], -1, -1, ref[3][1]]
    assert not got[1:3].any()
    for b in (0, 3):
        assert np.array_equal(got[b, :len(ref[b][0])], np.frombuffer(ref[b][0], np.uint8))


def test_models_create_refuses_a_non_monotonic_table(torch_cuda):
    from fpcodec_amd import _lib, bitstream
    models = draw(SIZES["full"], 1, 1, 0, True)[1]
    cum, h = models.cum_array(), C.c_void_p()
    cum[10] = cum[9]
    rc = _lib.lib().fpc_entropy_models_create(bitstream._sizes_arg(SIZES["full"]), cum.ctypes.data, C.byref(h))
    assert rc == -1 and not h.value and b"increasing" in _lib.lib().fpc_last_error()


def test_encoder_to_bytes_to_decoder_on_the_device(torch_cuda, synth, tmp_path):
    """Wavernn.encoder -> pack_batch -> unpack_batch -> decode_indices: the encoder's c_in bit for bit, the symbols a device
    tensor all the way"""
    torch = torch_cuda
    from fpcodec_amd import bitstream
    from fpcodec_amd.vq_func import load_codebooks
    from fpcodec_amd.wavernn import Wavernn
    cfg = {}
    for key, name in (("scl_cb_path", "scl_hi"), ("cb_path", "vq_hi"), ("bl_scl_cb_path", "scl_lo"), ("bl_cb_path", "vq_lo")):
        cfg[key] = os.path.join(tmp_path, name + ".npy")
        np.save(cfg[key], synth.codebooks()[name])
    model = Wavernn(in_features=20, gru_units1=384, gru_units2=128, fc_units=18)
    model.load_state_dict(synth.predictor_state_dict())
    feat = torch.from_numpy(synth.predictor_features(5, 90, utt0=800)).cuda()
    c_in, _, _, _, ind1, ind2, cb_tot, idx = model.encoder(cfg, feat, None, 0.09, 0.28, qtz=True, return_indices=True)
    sizes = load_codebooks(cfg["cb_path"], cfg["scl_cb_path"], cfg["bl_cb_path"], cfg["bl_scl_cb_path"]).sizes
    for models in (None, bitstream.Models(sizes, cb_tot, (float(ind1.mean()), float(ind2.mean())))):
        data, nbits = bitstream.pack_batch(idx, sizes, models)
        back = bitstream.unpack_batch(data, 90, sizes, models)
        assert back.is_cuda and int(nbits.min()) > 0 and torch.equal(back, idx)
        assert torch.equal(model.decode_indices(cfg, back, feat[:, :, 18:20]), c_in)
