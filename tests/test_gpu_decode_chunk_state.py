"""k_decode (one utterance per workgroup, set_pairing(-1)) in chunks of ONE frame: every frame border goes through the
per-stream state record.  The de-emphasis state in that record is written by the wave that tracks it (wave 3 with
FPC_PCM_WHERE 2, the drawing wave otherwise); a record written by another wave carries the value the chunk started from,
and every sample behind the first border differs.  The rest of the suite runs k_decode chunked only with chunks of 2 and 4
frames; chunks of one frame it runs on k_decode2 alone.  Instances 408, 208 and 1616, bit for bit against the CPU oracle."""
import numpy as np
import pytest

import vocoder_patterns as vp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,variant", [("default", 408), ("ladder", 208), ("widest_group", 1616)])
def test_one_frame_chunks_one_utterance_per_workgroup(synth, oracle, name, variant):
    from fpcodec_amd import _lib
    from fpcodec_amd.lpcnet import LPCNet
    _lib.require_gpu()
    w = synth.lpcnet_weights() if name == "default" else vp.build(synth, name)[0]
    voc, orc = LPCNet(w), oracle.LPCNet(w)
    assert voc.kernel_variant() == variant
    B, T = 3, 4
    f = synth.vocoder_features_raw(B, T, utt0=320)
    f[:, :, 20:] = oracle.ceps2lpc(f.reshape(-1, 36)[:, :20])[0].reshape(B, T, 16)
    f[:, :, 19] = -0.4
    f[:, 2, 19] = 0.9        # one voiced frame (the fifth barrier) between unvoiced ones
    sd = synth.seeds(B, utt0=320)
    ref = np.stack([orc.synthesize(f[b], int(sd[b])) for b in range(B)])
    assert int(np.abs(ref.astype(np.int32)).max()) > 100     # the material is not silence
    voc.set_pairing(-1)
    for chunk in (1, 0):
        voc.set_chunk_frames(chunk)
        pcm = voc.synthesize(f, sd).cpu().numpy()
        assert voc.last_streams_per_workgroup() == 1
        nz = np.argwhere(pcm != ref)
        assert nz.size == 0, f"{name}, chunk {chunk}: {len(nz)} samples differ, first at (utterance, sample) {nz[:3].tolist()}"
