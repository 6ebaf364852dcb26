"""Host side of the WaveNet's time-parallel pass on a handle of shapes alone: needs no device."""
import pytest

KW = dict(out_channels=2, num_blocks=2, num_layers=10, inp_channels=3, residual_channels=128, gate_channels=256,
          skip_channels=128, kernel_size=2, cin_channels=100, cout_channels=128, upsample_scales=[10, 16], local=False)


def test_forward_workspace_and_tile_on_a_shape_only_handle():
    from fpcodec_amd import _lib
    from fpcodec_amd.wavenet import Wavenet
    m = Wavenet(**KW)
    N = 160 * 3
    one = 4 * (128 * N + 12 * 3 * 128 + 2 * 128 * N + 128 * N + 3 * N)
    assert m.forward_workspace_bytes(1, 3) == one
    assert m.forward_workspace_bytes(5, 3) == 5 * one and m.forward_workspace_bytes(5, 6) == 10 * one
    assert m.forward_workspace_bytes(0, 3) == _lib.lib().fpc_wavenet_forward_workspace_bytes(None, 1, 1) < 0
    assert m.forward_tile() == 32 and Wavenet(tn=64, **KW).forward_tile() == 64
    # 512-wide panels fit at 16 positions only
    wide = dict(KW, residual_channels=512, gate_channels=512, skip_channels=512, cout_channels=512)
    assert Wavenet(**wide).forward_tile() == 16
    with pytest.raises(_lib.FpcError, match="LDS"):
        Wavenet(tn=32, **wide)
    with pytest.raises(_lib.FpcError, match="not 0, 16, 32 or 64"):
        Wavenet(tn=48, **KW)
    # the launch calls refuse a handle without weights before they touch any pointer
    for call, nptr in ((_lib.lib().fpc_wavenet_forward_parallel, 3), (_lib.lib().fpc_wavenet_forward_input, 2)):
        assert call(m.handle, *[None] * 3, 1, 1, *[None] * nptr, None) < 0
        assert b"without weights" in _lib.lib().fpc_last_error()
