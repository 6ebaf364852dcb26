"""The reference's own vocoder: the Gaussian-output WaveNet of src/models/wavenet.py, decoded by k_wn_decode
(csrc/wavenet_decode.h) for a whole batch of utterances, and evaluated teacher-forced over all positions at once by the k_wnf_*
kernels (csrc/wavenet_forward.h); `loss_backward` adds the Gaussian loss and the backward pass of the sample-level network
(k_wnb_*, csrc/wavenet_backward.h).  `Wavenet` takes the reference's constructor arguments and its
state_dict, key for key; `forward`, `generate_lpc`, `upsample` and `forward_stats` take the reference's tensor layouts."""
import ctypes as C

import numpy as np
import torch

from . import _lib

FRAME = 160


_NORMED = ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1"))
# ABI name of a sample-level weight -> the reference's module name ({} = "res_blocks.n.")
_MODULES = {"front": "front_conv.0.conv", "filter": "{}filter_conv.conv", "gate": "{}gate_conv.conv",
            "filter_c": "{}filter_conv_c", "gate_c": "{}gate_conv_c", "res": "{}res_conv", "skip": "{}skip_conv",
            "final1": "final_conv.1.conv", "final2": "final_conv.3.conv"}


def _folded(sd, name):
    """weight of module `name`: weight_norm's (g, v) pair folded with torch's own operator, or a plain weight"""
    for g, v in ((name + ".weight_g", name + ".weight_v"),
                 (name + ".parametrizations.weight.original0", name + ".parametrizations.weight.original1")):
        if g in sd:
            return torch._weight_norm(torch.as_tensor(sd[v]).float(), torch.as_tensor(sd[g]).float(), 0)
    return torch.as_tensor(sd[name + ".weight"]).float()


class Wavenet:
    def __init__(self, out_channels=1, num_blocks=3, num_layers=10, inp_channels=1, residual_channels=512,
                 gate_channels=512, skip_channels=512, kernel_size=2, cin_channels=36, cout_channels=36,
                 upsample_scales=None, causal=True, local=True, fat_upsampler=True, nu=0, tn=0):
        """wavenet.py:12-15; nu: utterances per workgroup of the sample loop (16, 32, 0 = chosen from the batch size); tn:
        positions per workgroup of the time-parallel pass (16, 32, 64, 0 = 32 where it fits the LDS, else 16).  Raises FpcError for a
        configuration the kernel does not serve (fpc_wavenet_config in include/fpcodec.h)."""
        scales = list(upsample_scales or [])
        if len(scales) != 2:
            raise _lib.FpcError(f"fpc_wavenet: upsample_scales = {scales}; only [10, 16] is built")
        self.cfg = _lib.WavenetConfig(out_channels, num_blocks, num_layers, inp_channels, residual_channels, gate_channels,
                                      skip_channels, kernel_size, cin_channels, cout_channels, (C.c_int * 2)(*scales),
                                      int(causal), int(local), int(fat_upsampler), nu)
        self.handle = None
        self.w = None
        self._ws = None
        self._fws = None
        self._bws = None
        self._gv = {}  # module name -> (key of g, key of v, g, v) on the device, where the state_dict was weight-normed
        self.tn = tn
        self._create(None)
        self.nfeat = cin_channels - 64
        self.layers = num_blocks * num_layers

    def _create(self, weights):
        h = C.c_void_p()
        _lib.check(_lib.lib().fpc_wavenet_create(C.byref(self.cfg), C.byref(weights) if weights is not None else None, C.byref(h)),
                   "fpc_wavenet_create")
        self._destroy()
        self.handle = h
        _lib.check(_lib.lib().fpc_wavenet_set_forward_tile(h, self.tn), "fpc_wavenet_set_forward_tile")

    def _destroy(self):
        if self.handle is not None:
            _lib.lib().fpc_wavenet_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def receptive_field_size(self):
        return sum(2 ** (i % self.cfg.num_layers) for i in range(self.layers)) + 32

    def load_state_dict(self, sd):
        """the reference's own keys (torch tensors or arrays); weight_g / weight_v pairs are folded here"""
        _lib.require_gpu()
        c = self.cfg
        R, G, S, co = c.residual_channels, c.gate_channels, c.skip_channels, c.cout_channels
        t = lambda k: torch.as_tensor(sd[k]).float()
        per_layer = lambda f: torch.stack([f(f"res_blocks.{n}.") for n in range(self.layers)])
        w = {
            "embedding": t("embedding.weight"),
            "c_conv0_w": t("c_conv.0.weight"), "c_conv0_b": t("c_conv.0.bias"),
            "c_conv1_w": t("c_conv.2.weight"), "c_conv1_b": t("c_conv.2.bias"),
            "c_fc0_w": t("c_fc.0.weight"), "c_fc0_b": t("c_fc.0.bias"),
            "c_fc1_w": t("c_fc.2.weight"), "c_fc1_b": t("c_fc.2.bias"),
            "up0_w": _folded(sd, "upsample_conv.0"), "up0_b": t("upsample_conv.0.bias"),
            "up1_w": _folded(sd, "upsample_conv.2"), "up1_b": t("upsample_conv.2.bias"),
            "front_w": _folded(sd, "front_conv.0.conv"), "front_b": t("front_conv.0.conv.bias"),
            "final1_w": _folded(sd, "final_conv.1.conv"), "final1_b": t("final_conv.1.conv.bias"),
            "final2_w": _folded(sd, "final_conv.3.conv"), "final2_b": t("final_conv.3.conv.bias"),
        }
        for key, mod in (("filter", "filter_conv.conv"), ("gate", "gate_conv.conv"), ("filter_c", "filter_conv_c"),
                         ("gate_c", "gate_conv_c"), ("res", "res_conv"), ("skip", "skip_conv")):
            w[key + "_w"] = per_layer(lambda p: _folded(sd, p + mod))
            w[key + "_b"] = per_layer(lambda p: t(p + mod + ".bias"))
        L = self.layers
        shapes = {"embedding": (256, 64), "c_conv0_w": (co, c.cin_channels, 3), "c_conv1_w": (co, co, 3),
                  "c_fc0_w": (co, co), "c_fc1_w": (co, co), "up0_w": (1, 1, 3, 20), "up1_w": (1, 1, 3, 32),
                  "front_w": (R, c.inp_channels, 32), "filter_w": (L, G, R, 2), "gate_w": (L, G, R, 2),
                  "filter_c_w": (L, G, co, 1), "gate_c_w": (L, G, co, 1), "res_w": (L, R, G, 1), "skip_w": (L, S, G, 1),
                  "final1_w": (S, S, 1), "final2_w": (2, S, 1)}
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"{k}: shape {tuple(w[k].shape)} != {s}")
        self.w = {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in w.items()}
        self._create(_lib.WavenetWeights(*[self.w[k].ctypes.data for k in _lib.WAVENET_KEYS]))
        self._gv = {}
        for mod in _MODULES.values():
            for name in ([mod.format(f"res_blocks.{n}.") for n in range(L)] if "{}" in mod else [mod]):
                for kg, kv in _NORMED:
                    if name + kg in sd:
                        self._gv[name] = (name + kg, name + kv, torch.as_tensor(sd[name + kg]).float().cuda(),
                                          torch.as_tensor(sd[name + kv]).float().cuda())
        return self

    # ---- calls ----
    def workspace_bytes(self, B, T):
        return int(_lib.lib().fpc_wavenet_workspace_bytes(self.handle, B, T))

    def _workspace(self, B, T):
        need = self.workspace_bytes(B, T)
        if need < 0:
            _lib.check(need, "fpc_wavenet_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        return self._ws

    def forward_workspace_bytes(self, B, T):
        return int(_lib.lib().fpc_wavenet_forward_workspace_bytes(self.handle, B, T))

    def set_forward_tile(self, tn):
        _lib.check(_lib.lib().fpc_wavenet_set_forward_tile(self.handle, tn), "fpc_wavenet_set_forward_tile")
        self.tn = tn

    def forward_tile(self):
        """positions per workgroup the time-parallel pass runs with"""
        return int(_lib.lib().fpc_wavenet_forward_tile(self.handle))

    def _forward_workspace(self, B, T):
        need = self.forward_workspace_bytes(B, T)
        if need < 0:
            _lib.check(need, "fpc_wavenet_forward_workspace_bytes")
        if self._fws is None or self._fws.numel() < need:
            self._fws = None
            self._fws = torch.empty(need, dtype=torch.uint8, device="cuda")
        return self._fws

    def _inputs(self, feat, periods, lpc):
        """reference layouts -> the ABI's: feat (B,nfeat,L) -> [B,L,nfeat]; periods (B,L,1) or (B,L) int; lpc per sample
        (B,160L,16), as synthesis.py:105 repeats it, or per frame (B,L,16)"""
        f = torch.as_tensor(feat).to("cuda", torch.float32).transpose(1, 2).contiguous()
        B, T, nf = f.shape
        if nf != self.nfeat:
            raise ValueError(f"feat has {nf} channels, the model takes {self.nfeat}")
        p = torch.as_tensor(periods).to("cuda", torch.int32).reshape(B, T).contiguous()
        a = None
        if lpc is not None:
            a = torch.as_tensor(lpc).to("cuda", torch.float32)
            if a.shape[1] == T * FRAME:
                a = a[:, ::FRAME]
            a = a.reshape(B, T, 16).contiguous()
        return f, p, a, B, T

    def upsample(self, c, periods):
        """wavenet.py:93-115: c (B,nfeat,L), periods (B,L,1) -> (B,cout,160L)"""
        f, p, _, B, T = self._inputs(c, periods, None)
        out = torch.empty(B, self.cfg.cout_channels, T * FRAME, device="cuda")
        ws = self._workspace(B, T)
        _lib.check(_lib.lib().fpc_wavenet_condition(self.handle, f.data_ptr(), p.data_ptr(), B, T, out.data_ptr(),
                                                    ws.data_ptr(), _lib.stream_ptr()), "fpc_wavenet_condition")
        return out

    def generate_lpc(self, feat, periods, lpc, seeds=None, noise=None, return_x=False):
        """wavenet.py:137-193 for a batch: (B,1,160L), the reference's x_out without its leading zero.  noise (B,160L):
        the standard normal draws to use; else Philox keyed by seeds (B,) (default 0..B-1).  return_x: also the reference's x
        buffer (the samples before line 188's filter), as a second (B,1,160L)."""
        f, p, a, B, T = self._inputs(feat, periods, lpc)
        if noise is not None:
            noise = torch.as_tensor(noise).to("cuda", torch.float32).reshape(B, T * FRAME).contiguous()
        sd = np.arange(B) if seeds is None else seeds
        sd = torch.as_tensor(np.asarray(sd).astype(np.int64) if not torch.is_tensor(sd) else sd)
        sd = sd.to("cuda", torch.int64).contiguous()
        assert sd.numel() == B
        out = torch.empty(B, 1, T * FRAME, device="cuda")
        x = torch.empty_like(out) if return_x else None
        ws = self._workspace(B, T)
        _lib.check(_lib.lib().fpc_wavenet_synthesize(
            self.handle, f.data_ptr(), p.data_ptr(), a.data_ptr(), B, T, sd.data_ptr(),
            noise.data_ptr() if noise is not None else None, out.data_ptr(), x.data_ptr() if return_x else None,
            ws.data_ptr(), _lib.stream_ptr()), "fpc_wavenet_synthesize")
        return (out, x) if return_x else out

    def forward(self, x, periods, c):
        """wavenet.py:83-91: x (B,inp_channels,160L), the net's own input channels, periods (B,L,1), c (B,nfeat,L) ->
        (B,2,160L).  All positions at once (k_wnf_*)."""
        f, p, _, B, T = self._inputs(c, periods, None)
        xs = torch.as_tensor(x).to("cuda", torch.float32).contiguous()
        if tuple(xs.shape) != (B, self.cfg.inp_channels, T * FRAME):
            raise ValueError(f"x has shape {tuple(xs.shape)}, not {(B, self.cfg.inp_channels, T * FRAME)}")
        st = torch.empty(B, T * FRAME, 2, device="cuda")
        ws = self._forward_workspace(B, T)
        _lib.check(_lib.lib().fpc_wavenet_forward_input(self.handle, f.data_ptr(), p.data_ptr(), xs.data_ptr(), B, T,
                                                        st.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
                   "fpc_wavenet_forward_input")
        return st.transpose(1, 2)

    __call__ = forward

    def backward_workspace_bytes(self, B, T):
        return int(_lib.lib().fpc_wavenet_backward_workspace_bytes(self.handle, B, T))

    def set_backward_tile(self, tn):
        """positions per workgroup of the backward's data-gradient kernels: 16, 32, 0 = automatic"""
        _lib.check(_lib.lib().fpc_wavenet_set_backward_tile(self.handle, tn), "fpc_wavenet_set_backward_tile")

    def backward_tile(self):
        return int(_lib.lib().fpc_wavenet_backward_tile(self.handle))

    def loss_backward(self, x, periods, c, target, n_valid=None, return_stats=False):
        """train.py:137-140 without the optimiser: forward(x, periods, c), gaussianloss(dist[:, :, :-1], target[:, :, 1:]) and
        its backward through the sample-level network.  x (B,inp_channels,160L), target (B,1,160L) or (B,160L) (the reference's
        exc); n_valid: positions of every utterance that count (default all 160L - 1).  -> (loss, grads): loss a 0-d tensor,
        grads keyed by the reference's state_dict names (weight_g / weight_v where the loaded state_dict had them, by
        weight_norm's closed form; else weight) plus "cfeat" (B,cout,160L), the gradient of upsample(c, periods).
        return_stats: also the (B,2,160L) stats of this pass, forward()'s bits."""
        f, p, _, B, T = self._inputs(c, periods, None)
        N, cfg, L = T * FRAME, self.cfg, self.layers
        xs = torch.as_tensor(x).to("cuda", torch.float32).contiguous().clone()
        if tuple(xs.shape) != (B, cfg.inp_channels, N):
            raise ValueError(f"x has shape {tuple(xs.shape)}, not {(B, cfg.inp_channels, N)}")
        y = torch.as_tensor(target).to("cuda", torch.float32).reshape(B, N)
        y = torch.cat((y[:, 1:], y.new_zeros(B, 1)), 1).contiguous()  # position p is scored against target[p + 1]
        n_valid = N - 1 if n_valid is None else int(n_valid)
        if not 1 <= n_valid <= N - 1:
            raise ValueError(f"n_valid = {n_valid} outside [1, {N - 1}]")
        R, G, S, co = cfg.residual_channels, cfg.gate_channels, cfg.skip_channels, cfg.cout_channels
        shapes = {"front_w": (R, cfg.inp_channels, 32), "front_b": (R,), "filter_w": (L, G, R, 2), "gate_w": (L, G, R, 2),
                  "filter_c_w": (L, G, co, 1), "gate_c_w": (L, G, co, 1), "res_w": (L, R, G, 1), "skip_w": (L, S, G, 1),
                  "res_b": (L, R), "skip_b": (L, S), "final1_w": (S, S, 1), "final1_b": (S,), "final2_w": (2, S, 1),
                  "final2_b": (2,), "cfeat": (B, co, N)}
        g = {k: torch.empty(shapes.get(k, (L, G)), device="cuda") for k in _lib.WAVENET_GRAD_KEYS}
        loss = torch.empty((), device="cuda")
        need = self.backward_workspace_bytes(B, T)
        if need < 0:
            _lib.check(need, "fpc_wavenet_backward_workspace_bytes")
        if self._bws is None or self._bws.numel() < need:
            self._bws = None
            self._bws = torch.empty(need, dtype=torch.uint8, device="cuda")
        gs = _lib.WavenetGrads(*[g[k].data_ptr() for k in _lib.WAVENET_GRAD_KEYS])
        _lib.check(_lib.lib().fpc_wavenet_loss_backward(self.handle, f.data_ptr(), p.data_ptr(), xs.data_ptr(), y.data_ptr(),
                                                        n_valid, B, T, loss.data_ptr(), C.byref(gs), self._bws.data_ptr(),
                                                        _lib.stream_ptr()), "fpc_wavenet_loss_backward")
        out = {"cfeat": g["cfeat"]}
        for key, mod in _MODULES.items():
            for n in (range(L) if "{}" in mod else [None]):
                name = mod.format(f"res_blocks.{n}.")
                dw, db = (g[key + "_w"], g[key + "_b"]) if n is None else (g[key + "_w"][n], g[key + "_b"][n])
                out[name + ".bias"] = db
                if name not in self._gv:
                    out[name + ".weight"] = dw
                    continue
                kg, kv, gg, v = self._gv[name]  # w = g v / |v|, the norm over all dimensions but 0
                dims = tuple(range(1, v.dim()))
                norm = v.pow(2).sum(dims, keepdim=True).sqrt()
                dot = (dw * v).sum(dims, keepdim=True)
                out[kg] = dot / norm
                out[kv] = (gg / norm) * (dw - v * dot / norm.pow(2))
        if return_stats:
            off = int(_lib.lib().fpc_wavenet_backward_stats_offset(self.handle, B, T))
            st = self._bws[off:off + 8 * B * N].view(torch.float32).reshape(B, N, 2).transpose(1, 2).clone()
            return loss, out, st
        return loss, out

    def forward_stats(self, x, feat, periods, lpc, time_parallel=False):
        """teacher-forced: x (B,1,160L) or (B,160L) -> (B,2,160L), (mean, log_std) of every sample given the ones before
        it -- Wavenet.forward on the inputs generate_lpc builds from x.  time_parallel: all positions at once (k_wnf_*)
        instead of the sample loop; the same values bit for bit."""
        f, p, a, B, T = self._inputs(feat, periods, lpc)
        xs = torch.as_tensor(x).to("cuda", torch.float32).reshape(B, T * FRAME).contiguous()
        st = torch.empty(B, T * FRAME, 2, device="cuda")
        if time_parallel:
            ws = self._forward_workspace(B, T)
            _lib.check(_lib.lib().fpc_wavenet_forward_parallel(self.handle, f.data_ptr(), p.data_ptr(), a.data_ptr(), B, T,
                                                               xs.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                                               _lib.stream_ptr()), "fpc_wavenet_forward_parallel")
            return st.transpose(1, 2)
        ws = self._workspace(B, T)
        _lib.check(_lib.lib().fpc_wavenet_forward(self.handle, f.data_ptr(), p.data_ptr(), a.data_ptr(), B, T,
                                                  xs.data_ptr(), st.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
                   "fpc_wavenet_forward")
        return st.transpose(1, 2)

    def last_decode_ms(self):
        return float(_lib.lib().fpc_wavenet_last_decode_ms(self.handle))
