"""Host side of the WaveNet's loss + backward call on a handle of shapes alone: needs no device."""
import ctypes as C

from test_wavenet_forward_cpu import KW


def test_backward_exports_workspace_and_refusals():
    from fpcodec_amd import _lib
    from fpcodec_amd.wavenet import Wavenet
    L = _lib.lib()
    for name in ("fpc_wavenet_loss_backward", "fpc_wavenet_backward_workspace_bytes", "fpc_wavenet_backward_stats_offset",
                 "fpc_wavenet_set_backward_tile", "fpc_wavenet_backward_tile"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    m = Wavenet(**KW)
    ws = m.backward_workspace_bytes
    # B T (160 (cout + 20 R + 20 2G + 4 S + 4 + 2G + 5 R) + 12 cout) + 2 B + 32 x 512 x 384 floats
    per_frame = 160 * (128 + 20 * 128 + 20 * 512 + 4 * 128 + 4 + 512 + 5 * 128) + 12 * 128
    assert ws(2, 3) == 4 * (6 * per_frame + 2 * 2 + 32 * 512 * 384)
    assert ws(3, 5) - ws(2, 5) == ws(2, 5) - ws(1, 5) and ws(3, 9) - ws(3, 6) == ws(3, 6) - ws(3, 3)
    assert ws(16, 10) == 1520779392
    assert ws(0, 3) == L.fpc_wavenet_backward_workspace_bytes(None, 1, 1) < 0
    assert m.backward_tile() == 32
    one = C.c_float()
    grads = _lib.WavenetGrads(*[C.addressof(one)] * len(_lib.WAVENET_GRAD_KEYS))
    ptr = C.addressof(one)
    call = lambda handle, n_valid: L.fpc_wavenet_loss_backward(handle, ptr, ptr, ptr, ptr, n_valid, 1, 1, ptr, C.byref(grads), ptr, None)
    assert call(None, 1) < 0 and b"null handle" in L.fpc_last_error()
    for n_valid in (0, 161):
        assert call(m.handle, n_valid) < 0 and b"n_valid" in L.fpc_last_error()
    assert call(m.handle, 160) < 0 and b"without weights" in L.fpc_last_error()  # refused before any pointer is touched
