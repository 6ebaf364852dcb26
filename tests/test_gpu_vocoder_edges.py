"""The vocoder's decode kernels (k_decode, k_decode2: csrc/lpcnet_decode.h, lpcnet_decode2.h) where the rest of the suite
does not reach: the launch that splits a batch between the two kernels (one pass and chunked), recurrent matrices built at
the edges of the block placement of fpc_lpcnet_create, and signals that saturate the table activations, the mu-law search,
the int16 output and the period index.  Every comparison is bit for bit with the CPU oracle."""
import numpy as np
import pytest

import vocoder_patterns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from fpcodec_amd import _lib
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def models(torch_cuda, synth, oracle):
    """name -> (device handle, oracle handle, weights, blocks kept per row group), built once: 'default' (no counts), or a
    pattern of tests/vocoder_patterns.py"""
    from fpcodec_amd.lpcnet import LPCNet
    cache = {}

    def get(name):
        if name not in cache:
            w, counts = (synth.lpcnet_weights(), None) if name == "default" else vocoder_patterns.build(synth, name)
            cache[name] = (LPCNet(w), oracle.LPCNet(w), w, counts)
        return cache[name]
    return get


@pytest.fixture
def restored():
    """handles a test has reconfigured go back to the default pairing and the one-pass form, whatever the test's end"""
    used = []
    yield used.append
    for voc in used:
        voc.set_pairing(0)
        voc.set_chunk_frames(0)


def _features(synth, oracle, B, T, utt0):
    f = synth.vocoder_features_raw(B, T, utt0=utt0)
    f[:, :, 20:] = oracle.ceps2lpc(f.reshape(-1, 36)[:, :20])[0].reshape(B, T, 16)
    return f


def _run(voc, f, sd, pairing, chunk):
    voc.set_pairing(pairing)
    voc.set_chunk_frames(chunk)
    pcm = voc.synthesize(f, sd).cpu().numpy()
    return pcm, voc.last_streams_per_workgroup()


def _same(got, want, what):
    nz = np.argwhere(got != want)
    assert nz.size == 0, f"{what}: {len(nz)} samples differ, first at (utterance, sample) {nz[:3].tolist()}"


def _oracle_rows(orc, f, sd, rows):
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(min(16, len(rows))) as ex:
        return list(ex.map(lambda b: orc.synthesize(f[b], int(sd[b])), rows))


# ------------------------------------------------------------------------------------------------------------------------
# A. split launches
# ------------------------------------------------------------------------------------------------------------------------
def _cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _predicted_pairs(B, cus):
    from fpcodec_amd import _lib
    return int(_lib.lib().fpc_lpcnet_paired_utterances(B, cus))


def test_mixed_launch_one_pass_and_chunked(torch_cuda, models, restored, synth, oracle):
    """a batch of 2 CUs + 8 distinct utterances: the first 2 CUs go two per workgroup on k_decode2, the last 8 one per
    workgroup on k_decode, whose launch gets every base shifted (features, seeds, PCM, both conditioning products and, in a
    chunked pass, the carried state records, with a chunk stride that is not T).  One pass, chunks of 2 and of 4 frames (a
    ragged last chunk) and one utterance per workgroup throughout must give the same samples, and the rows either side of
    the split the oracle's"""
    voc, orc, w, _ = models("default")
    restored(voc)
    cus = _cus(torch_cuda)
    B, T = 2 * cus + 8, 6
    NP = _predicted_pairs(B, cus)
    assert NP == 2 * cus
    f = _features(synth, oracle, B, T, utt0=5000)      # every utterance its own features and its own seed
    f[NP - 1, :, 19] = 0.9                             # voiced on both sides of the split ...
    f[NP, :, 19] = 0.9
    f[NP - 2, 0::2, 19], f[NP - 2, 1::2, 19] = 0.9, -0.4   # ... beside rows that alternate voiced and unvoiced frames
    f[NP + 1, 1::2, 19], f[NP + 1, 0::2, 19] = 0.9, -0.4
    sd = synth.seeds(B, utt0=5000)
    assert len({f[b].tobytes() for b in range(B)}) == B and len(set(sd.tolist())) == B
    one, s_one = _run(voc, f, sd, 0, 0)
    c2, s_c2 = _run(voc, f, sd, 0, 2)
    c4, s_c4 = _run(voc, f, sd, 0, 4)
    plain, s_plain = _run(voc, f, sd, -1, 0)
    assert (s_one, s_c2, s_c4, s_plain) == (2, 2, 2, 1)
    _same(c2, one, "chunks of 2 frames against one pass")
    _same(c4, one, "chunks of 4 frames against one pass")
    _same(plain, one, "one utterance per workgroup against the mixed launch")
    rows = (0, NP - 1, NP, B - 1)
    for b, ref in zip(rows, _oracle_rows(orc, f, sd, rows)):
        _same(one[b:b + 1], ref[None], f"utterance {b} against the oracle")
    assert int(np.abs(one[NP].astype(np.int32)).max()) > 100


def test_all_paired_over_two_rounds_odd_batch(torch_cuda, models, restored, synth, oracle):
    """3 CUs + 1 utterances: all of them go two per workgroup (a full round of k_decode2 and half of a second), and the last
    workgroup holds one utterance, which it decodes twice"""
    voc, orc, w, _ = models("default")
    restored(voc)
    cus = _cus(torch_cuda)
    B, T = 3 * cus + 1, 2
    assert _predicted_pairs(B, cus) == B
    f = _features(synth, oracle, B, T, utt0=7000)
    f[B - 1, :, 19] = 0.9
    f[2 * cus - 1, 0, 19] = 0.9
    sd = synth.seeds(B, utt0=7000)
    one, s_one = _run(voc, f, sd, 0, 0)
    c1, s_c1 = _run(voc, f, sd, 0, 1)
    plain, s_plain = _run(voc, f, sd, -1, 0)
    assert (s_one, s_c1, s_plain) == (2, 2, 1)
    _same(c1, one, "chunks of 1 frame against one pass")
    _same(plain, one, "one utterance per workgroup against two")
    rows = (0, 2 * cus - 1, 2 * cus, B - 1)
    for b, ref in zip(rows, _oracle_rows(orc, f, sd, rows)):
        _same(one[b:b + 1], ref[None], f"utterance {b} against the oracle")


# ------------------------------------------------------------------------------------------------------------------------
# B. weight patterns at the packing edges
# ------------------------------------------------------------------------------------------------------------------------
# pattern -> (kernel instance, two utterances per workgroup when asked), derived from the group widths by hand (lanes per
# group = max(1, ceil(blocks / 4)); 208: z, r <= 2 lanes and n <= 8; 408: z, r <= 4 and n <= 8; 1616 otherwise and never
# paired; pairing needs every group padded to an even width within 512 lanes).  The kept off-diagonal values are the dense
# matrix's own (rescaling constant 1.0 for every pattern: none saturates the voiced utterance or lets it die).
EXPECT = {
    "ladder": (208, True),
    "diagonal_crossing": (208, True),
    "diagonal_crossing_zero_diagonal": (208, True),
    "diagonal_only": (208, True),
    "edge_of_408": (408, True),
    "one_past_the_edge_z17": (1616, False),
    "one_past_the_edge_n33": (1616, False),
    "widest_group": (1616, False),
    "no_room_for_padding": (408, False),
    "skewed": None,      # whatever its drawn widths imply
}


def test_every_pattern_has_an_expectation():
    assert set(EXPECT) == set(vocoder_patterns.PATTERNS)


@pytest.mark.parametrize("name", list(EXPECT))
def test_packing_edge_pattern(torch_cuda, models, restored, synth, oracle, name):
    """an odd batch with an unvoiced, a voiced and two partly voiced utterances (the layout of
    test_lpcnet_two_utterances_per_workgroup_small), one and two utterances per workgroup, one pass and chunks of 2 frames:
    all equal to the oracle, on the instance and with the pairing the widths imply"""
    voc, orc, w, counts = models(name)
    restored(voc)
    implied = vocoder_patterns.expectation(counts)
    variant, pairs = EXPECT[name] or implied
    assert implied == (variant, pairs)     # the table above and the arithmetic agree on what is being asked
    B, T = 5, 5
    f = _features(synth, oracle, B, T, utt0=11)
    f[0, :, 19] = -0.4
    f[1, :, 19] = 0.9
    f[2, 1:3, 19] = 0.8
    f[3, 2:4, 19] = 0.7
    sd = synth.seeds(B, utt0=11)
    ref = np.stack(_oracle_rows(orc, f, sd, range(B)))
    live = int(np.abs(ref[1].astype(np.int32)).max())
    print(f"pattern {name}: {int(counts.sum())} blocks, widest z/r group {int(counts[:2].max())}, widest n group "
          f"{int(counts[2].max())}; instance {voc.kernel_variant()}, expected {variant}, pairs {pairs}; "
          f"max |pcm| of the voiced utterance {live}")
    assert live > 100
    assert voc.kernel_variant() == variant
    for pairing in (-1, 1):
        for chunk in (0, 2):
            pcm, streams = _run(voc, f, sd, pairing, chunk)
            assert streams == (2 if pairing == 1 and pairs else 1), (pairing, chunk, streams)
            _same(pcm, ref, f"pattern {name}, pairing {pairing}, chunk {chunk}")


def test_group_of_65_blocks_is_refused(torch_cuda, synth):
    """64 blocks fill the 16 lanes of a DPP row (pattern widest_group); one more has nowhere to go"""
    from fpcodec_amd._lib import FpcError
    from fpcodec_amd.lpcnet import LPCNet
    w, counts = vocoder_patterns.weights(synth, vocoder_patterns.TOO_WIDE)
    assert counts.max() == 65
    with pytest.raises(FpcError, match="too dense"):
        LPCNet(w)


# ------------------------------------------------------------------------------------------------------------------------
# C. the saturating regime
# ------------------------------------------------------------------------------------------------------------------------
def _both_kernels_equal_oracle(voc, orc, f, sd, what, paired=True):
    ref = np.stack(_oracle_rows(orc, f, sd, range(len(f))))
    for pairing in (-1, 1):
        pcm, streams = _run(voc, f, sd, pairing, 0)
        assert streams == (2 if pairing == 1 and paired else 1)
        _same(pcm, ref, f"{what}, pairing {pairing}")
    return ref


@pytest.mark.parametrize("name", ["default", "ladder"])      # instance 408 and instance 208 of both kernels
def test_unstable_lpc_saturates_ulaw_and_int16(torch_cuda, models, restored, synth, oracle, name):
    """a one-tap synthesis filter of radius 1.03: the signal leaves the int16 range within the first frame and grows for
    four (1.03^640 = 1.6e8 times the excitation it starts from: finite in float32).  Past +-32768 the mu-law search sits on
    its clamps (K > 128, u > 255; k_decode2 restates it as ulaw_issue / ulaw_finish) and fpc_pcm16 on the int16 limits"""
    voc, orc, w, _ = models(name)
    restored(voc)
    B, T = 4, 4
    f = _features(synth, oracle, B, T, utt0=21)
    f[1, :, 19] = f[3, :, 19] = 0.9
    f[:, :, 20:] = 0.0
    f[:2, :, 20] = -1.03     # prediction = 1.03 x the last sample: monotone growth
    f[2:, :, 20] = 1.03      # the sign alternates every sample
    sd = synth.seeds(B, utt0=21)
    # the material does what it is for (CPU): checked before anything runs on the device
    limits, levels, peak = set(), set(), 0.0
    for b in range(B):
        pcm, exc, pf = orc.synthesize(f[b], int(sd[b]), trace=True)
        assert np.isfinite(pf).all()
        peak = max(peak, float(np.abs(pf).max()))
        assert np.abs(pf).max() > 32768
        limits |= {int(v) for v in (pcm.min(), pcm.max())}
        below = {int(oracle.lib().orc_lin2ulaw(float(x))) for x in pf[pf < -32768]}
        above = {int(oracle.lib().orc_lin2ulaw(float(x))) for x in pf[pf > 32768]}
        assert below <= {0} and above <= {255}, (b, below, above)
        levels |= below | above
    print(f"unstable LPC, {name}: largest |float pcm| of the oracle {peak:.4g}")
    assert {-32768, 32767} <= limits and levels == {0, 255}
    _both_kernels_equal_oracle(voc, orc, f, sd, f"unstable LPC, weights {name}")


@pytest.mark.parametrize("name", ["default", "ladder"])
def test_saturated_table_activations(torch_cuda, synth, oracle, name):
    """the biases of both GRUs and of the dual FC times 40 (the factor is not lowered: the draws stay spread over many
    levels).  The dual FC's biases become +-48 with a sigma of 12, so nearly all of its tanh arguments lie beyond |x| = 8,
    where the table index min(|x| * scale, 4095.99976) sits on its clamp -- k_decode's lut_scaled, k_decode2's lut_issue /
    lut_finish; the GRUs' folded biases get a sigma of 2 to 2.8, which drives their gates into the flat top of the table
    (the sigmoid's clamp at |x| = 16 is six sigma out: the oracle exposes no pre-activation to tell whether one gets there)"""
    from fpcodec_amd.lpcnet import LPCNet
    w = dict(synth.lpcnet_weights() if name == "default" else vocoder_patterns.build(synth, name)[0])
    for k in ("gru_a_bias", "gru_b_bias", "md_bias"):
        w[k] = (w[k] * np.float32(40.0)).astype(np.float32)
    voc, orc = LPCNet(w), oracle.LPCNet(w)
    B, T = 4, 4
    f = _features(synth, oracle, B, T, utt0=31)
    f[1, :, 19] = 0.9
    sd = synth.seeds(B, utt0=31)
    peak = 0.0
    for b in range(B):      # the oracle exposes no pre-activations: what it does expose must not have collapsed
        pcm, exc, pf = orc.synthesize(f[b], int(sd[b]), trace=True)
        assert np.isfinite(pf).all()
        assert len(set(exc[17:].tolist())) > 1
        peak = max(peak, float(np.abs(pf).max()))
    print(f"saturated activations, {name}: largest |float pcm| of the oracle {peak:.4g}")
    _both_kernels_equal_oracle(voc, orc, f, sd, f"biases x 40, weights {name}")


@pytest.mark.parametrize("name", ["default", "ladder"])
def test_period_index_clamps(torch_cuda, models, restored, synth, oracle, name):
    """feature 18 far outside the range of the pitch embedding (both clamps of fpc_period_index), on the last values that
    need no clamp (0.1f + 50 x + 100 = -7.6e-6 and 255.00002 in float32: indices 0 and 255) and one index inside them"""
    voc, orc, w, _ = models(name)
    restored(voc)
    values = (-3.0, 4.0, -2.002, 3.098, -1.98, 3.08)
    assert [oracle.period_index(v) for v in values] == [0, 255, 0, 255, 1, 254]
    f32 = np.float32
    assert [int(np.clip(int(f32(f32(f32(0.1) + f32(50.0) * f32(v)) + f32(100.0))), 0, 255)) for v in values] == \
        [0, 255, 0, 255, 1, 254]
    B, T = 4, 4
    f = _features(synth, oracle, B, T, utt0=41)
    f[0, :, 18] = values[:4]                 # every value at the first and at the last frame of some utterance (the k=3
    f[1, :, 18] = values[:4][::-1]           # convolutions' zero padding beside it) and inside one
    f[2, :, 18] = values[4:] + values[:2]
    f[3, 1, 19] = 0.9
    sd = synth.seeds(B, utt0=41)
    cfeat = voc.condition(f).cpu().numpy()
    for b in range(B):
        assert np.array_equal(cfeat[b], orc.condition(f[b])), f"conditioning vectors of utterance {b}"
    _both_kernels_equal_oracle(voc, orc, f, sd, f"period-index clamps, weights {name}")
