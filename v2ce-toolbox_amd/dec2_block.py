"""The first half of the third decoder block -- the spectral-normalised 3x3x3 ``conv1`` and the 1x1x1 shortcut convolution
``downsample.0`` of ``UNet.decoders[2]``, both ``Conv3d(192, 64)`` on ``cat(nearest_upsample_2x(dec1 output), skip)``, with
the affine parts of ``bn1`` / ``downsample.1`` -- as trainable layers on the GPU, the whole block as one layer, and the
weight gradients through the upsample + concat at any of the decoders' channel counts that they stand on
(include/v2ce_hip_convupngrad.h, csrc/convupnwgrad.hip): the checked entry ``convupn_wgrad``.

    h1, s2, x1 = model.forward_dec2_sources(x)    # the frozen trunk up to dec2's two sources and dec3's skip tensor
    dec2 = Dec2Block.from_model(model)            # Dec2Convs -> Dec2Norms -> Dec2Conv: ten parameter tensors
    block, head = LastBlock.from_model(model), PredHead.from_model(model)
    pred = head(block(dec2(h1, s2), x1))          # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # dec2.convs.weight_bar.grad, dec2.convs.short_weight.grad, ...
    for m in (dec2, block, head): m.write_back(model)

With ``Dec2Conv`` (dec2_conv.py) this is the reference's whole ``ResidualBlock3D(192, 64, norm='BN', sn=True)``
(train/scripts/model/submodules.py:249-264) at half the output resolution.  The channel counts of ``convupn_wgrad`` are read
from the tensors; 64 + 32 -> 32 restates ``last_block.convup_wgrad`` byte for byte.  The gradient with respect to the two
sources (a ``v2ce_convup_dgrad`` at 192 -> 64) has no consumer until ``UNet.decoders[1].conv2`` trains and is not provided:
``Dec2Convs`` refuses sources that require grad.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .dec2_conv import Dec2Conv
from .last_conv import _planar_pitched
from .pred_head import _check_f32, _no_overlap

C = 64                     # output channels of dec2.conv1 and of the shortcut
C0, C1 = 128, 64           # upsampled channels, skip channels
CIN = C0 + C1
TAPS = 27
WANT = ("weight", "short", "short_bias")


def _check_c16(t, name, channels):
    """-> (C, B, L, H, W, pitch) of a channels-last-16 tensor whose channel count is one of ``channels``."""
    _check_f32(t, name)
    if t.dim() != 6 or t.shape[5] != 16 or int(t.shape[2]) * 16 not in channels:
        raise ValueError(f"{name} must be channels-last-16 [b, l, c / 16, h, pitch, 16] with c in {tuple(channels)}, got "
                         f"{tuple(getattr(t, 'shape', ()))}")
    B, L, G, H, pitch, _ = (int(v) for v in t.shape)
    W = int(getattr(t, "lw", pitch))
    if not 1 <= W <= pitch:
        raise ValueError(f"{name}.lw = {W} is outside 1 .. pitch = {pitch}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return G * 16, B, L, H, W, pitch


def _check_sources(x0, x1):
    """x0 at the source resolution against x1: the same b and l, h0 = (h + 1) // 2, lw0 = (lw + 1) // 2 and a nearest
    upsample that reads its source at (h >> 1, w >> 1) -> (c0, c1, B, L, H, W, pitch, pitch0)."""
    from .v2ce_3d import _nearest_is_half
    c1, B, L, H, W, pitch = _check_c16(x1, "x1", hip.CONVUPN_C1)
    c0, B0, L0, H0, W0, pitch0 = _check_c16(x0, "x0", hip.CONVUPN_C0)
    if x0.device != x1.device:
        raise ValueError(f"x0 lives on {x0.device}, x1 on {x1.device}")
    if (B0, L0) != (B, L) or H0 != (H + 1) // 2 or W0 != (W + 1) // 2:
        raise ValueError(f"x0 {tuple(x0.shape)} (lw {W0}) must match x1 {tuple(x1.shape)} (lw {W}): the same b and l, "
                         f"h0 = (h + 1) // 2 = {(H + 1) // 2} and lw = {(W + 1) // 2}")
    if not (_nearest_is_half(H0, H) and _nearest_is_half(W0, W)):
        raise ValueError(f"the nearest upsample {(H0, W0)} -> {(H, W)} does not read its source at (h >> 1, w >> 1)")
    return c0, c1, B, L, H, W, pitch, pitch0


def convupn_wgrad(x0: torch.Tensor, x1: torch.Tensor, g1: Optional[torch.Tensor], gd: Optional[torch.Tensor], *,
                  want: Sequence[str] = WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradients of the 3x3x3 and the 1x1x1 convolution c0 + c1 -> cout on the virtual tensor
    ``X = cat(nearest_upsample_2x(x0), x1)``.  ``x0`` is channels-last-16 ``[B, L, c0 / 16, H0, pitch0, 16]`` f32 (c0 = 64
    or 128) with ``H0 = (H + 1) // 2`` and ``.lw = (W + 1) // 2``; ``x1`` (the skip tensor, c1 = 32 or 64 channels) is
    ``[B, L, c1 / 16, H, pitch, 16]``; ``g1`` (the gradient with respect to the 3x3x3 convolution's output) and ``gd`` (the
    gradient with respect to the 1x1x1 convolution's output) are ``[B, L, cout / 16, H, pitch, 16]`` (cout = 32 or 64) with
    ``x1``'s B, L, H, pitch and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'short', 'short_bias'): 'weight'
    [cout, c0 + c1, 3, 3, 3] = sum over the positions of g1[co] X[ci] shifted by the tap (zero padding at the upsampled
    resolution), 'short' [cout, c0 + c1] = sum of gd[co] X[ci], 'short_bias' [cout] = sum of gd[co].  ``g1`` may be None
    without 'weight', ``gd`` without 'short' and 'short_bias'.  ``out``: {name: tensor} to write into.  ``max_workgroups``:
    0 = the kernel's choice, n > 0 caps the shares of the tile walk at max(n / pairs, 1), pairs = (cout / 32)
    ((c0 + c1) / 32) (the result then depends on n only through the order of the f64 sums).  One call, no host
    synchronisation."""
    want = tuple(want)
    if not want or any(n not in WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    if "weight" in want and g1 is None:
        raise ValueError("want 'weight' needs g1")
    if ("short" in want or "short_bias" in want) and gd is None:
        raise ValueError("want 'short' and 'short_bias' need gd")
    c0, c1, B, L, H, W, pitch, pitch0 = _check_sources(x0, x1)
    dev = x1.device
    ins, cout = [("x0", x0), ("x1", x1)], None
    for n, t in (("g1", g1), ("gd", gd)):
        if t is None:
            continue
        co, *pos = _check_c16(t, n, hip.CONVUPN_COUT)
        if t.device != dev:
            raise ValueError(f"{n} lives on {t.device}, x1 on {dev}")
        if tuple(pos) != (B, L, H, W, pitch):
            raise ValueError(f"{n} {tuple(t.shape)} (lw {pos[3]}) must match x1 {tuple(x1.shape)} (lw {W}) but for the planes")
        if cout is not None and co != cout:
            raise ValueError(f"gd {tuple(t.shape)} must match g1 {tuple(g1.shape)}")
        cout = co
        ins.append((n, t))
    cin = c0 + c1
    shapes = {"weight": (cout, cin, 3, 3, 3), "short": (cout, cin), "short_bias": (cout,)}
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if t.numel() != torch.Size(shapes[n]).numel():
            raise ValueError(f"out['{n}'] has {t.numel()} elements")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_convupn_wgrad_workspace_bytes(c0, c1, cout, B, L, H, W, pitch, pitch0, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_convupn_wgrad: unsupported shape {(B, L, H, W)} (pitch {pitch}, pitch0 {pitch0}, "
                               f"{c0} + {c1} -> {cout})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {n: out[n] if n in out else torch.empty(shapes[n], dtype=torch.float32, device=dev) for n in want}
        hip.check(lib.v2ce_convupn_wgrad(x0.data_ptr(), x1.data_ptr(), hip.ptr(g1) if "weight" in want else None,
                                         hip.ptr(gd) if ("short" in want or "short_bias" in want) else None,
                                         c0, c1, cout, B, L, H, W, pitch, pitch0, hip.ptr(res.get("weight")),
                                         hip.ptr(res.get("short")), hip.ptr(res.get("short_bias")), ws.data_ptr(), nb,
                                         int(max_workgroups), hip.stream_ptr(dev)), "v2ce_convupn_wgrad")
    return res


class _Dec2ConvsFn(torch.autograd.Function):
    """forward: z1 = rs1 conv1(X; W_bar / sigma) + shift1 and zd = rsd conv_d(X; Wd) + shift_d as the model's own two
    launches on X = cat(upsample(x0), x1) -- conv1's and the shortcut's own 1x1x1 launch, in either precision -- on planes
    packed from W_bar with the sigma of the layer's power iteration, and from Wd; backward: one v2ce_convupn_wgrad call on
    the gradients of (z1, zd), then dW = rs1[co] dM1[co], dWd = rsd[co] dMd[co], d_bias_d = rsd[co] sum gd[co] (the
    normalisations are per output channel and linear, so they commute with the sums over the positions).  Nothing is
    launched when no parameter needs a gradient; x0 and x1 get none."""

    @staticmethod
    def forward(ctx, x0, x1, W, short_w, short_b, layer):
        model = layer._model[0]
        split = model.precision == "f16x2"
        dev = x1.device
        with torch.no_grad(), torch.cuda.device(dev):
            if model._prep is None:
                model._prepare()
            P = model._prep
            rs1 = (1.0 / torch.sqrt(layer.bn1_var + layer.eps)).float().contiguous()
            rsd = (1.0 / torch.sqrt(layer.bnd_var + layer.eps)).float().contiguous()
            shift1 = (-layer.bn1_mean * rs1).float().contiguous()
            shift_d = (-layer.bnd_mean * rsd if short_b is None else (short_b.detach() - layer.bnd_mean) * rsd).float().contiguous()
            w1, wd = layer._buffers_for(model, split, dev)
            model._pack(layer.weight_bar.detach().contiguous(), layer._sigma, w1, split=split)
            model._pack(short_w.detach().contiguous(), None, wd, split=split)
            up_to = (int(x1.shape[3]), int(getattr(x1, "lw", x1.shape[4])))
            # the launches take their range slots from the model's table: a table of this call's own, put back afterwards
            saved = (P["absmax"], getattr(model, "_slot", 0))
            P["absmax"], model._slot = torch.zeros((2, x1.shape[0], 2), dtype=torch.float32, device=dev), 0
            try:
                if split:
                    z1 = model._conv(x0, x1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=True)
                    zd = model._conv(x0, x1, wd, rsd, shift_d, C, 1, 1, hip.ACT_NONE, up_to=up_to, split=True)
                    torch.maximum(layer.guard, P["absmax"][:, :, 1].max().reshape(1), out=layer.guard)
                    del z1.absmax, zd.absmax              # (views of this call's table)
                else:
                    p0, p1 = _planar_pitched(x0), _planar_pitched(x1)
                    z1 = model.to_c16(model._conv(p0, p1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=False))
                    zd = model.to_c16(model._conv(p0, p1, wd, rsd, shift_d, C, 1, 1, hip.ACT_NONE, up_to=up_to, split=False))
            finally:
                P["absmax"], model._slot = saved
        ctx.save_for_backward(x0, x1, rs1, rsd)
        ctx.lw0, ctx.lw = getattr(x0, "lw", x0.shape[4]), up_to[1]
        for z in (z1, zd):
            z.lw, z.c16 = up_to[1], True
        return z1, zd

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, gd):
        x0, x1, rs1, rsd = ctx.saved_tensors
        _, _, need_w, need_sw, need_sb = ctx.needs_input_grad[:5]
        x0.lw, x1.lw = ctx.lw0, ctx.lw                  # (attributes do not survive save_for_backward on every version)
        want = (("weight",) if need_w and g1 is not None else ()) + (("short",) if need_sw and gd is not None else ()) + \
            (("short_bias",) if need_sb and gd is not None else ())
        if not want:
            return (None,) * 6
        if g1 is not None:
            g1 = g1.contiguous()
            g1.lw = ctx.lw
        if gd is not None:
            gd = gd.contiguous()
            gd.lw = ctx.lw
        r = convupn_wgrad(x0, x1, g1, gd, want=want)
        dW = rs1.view(C, 1, 1, 1, 1) * r["weight"] if "weight" in r else None
        d_sw = (rsd.view(C, 1) * r["short"]).view(C, CIN, 1, 1, 1) if "short" in r else None
        d_sb = rsd * r["short_bias"] if "short_bias" in r else None
        return None, None, dW, d_sw, d_sb, None


class Dec2Convs(nn.Module):
    """``UNet.decoders[2].conv1`` and ``.downsample[0]`` with the normalising halves of ``bn1`` and ``downsample[1]`` as a
    trainable module, the layer in ``.eval()``: ``TailConvs`` (last_block.py) at 128 + 64 -> 64.  The BatchNorm statistics
    are frozen buffers (their affine parts are ``Dec2Norms``'), conv1's ``weight_bar`` and the shortcut's weight (and bias,
    where the model has one) train.  Like the reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` /
    ``weight_v`` by one power iteration (no gradient; the model's own kernel ``v2ce_sn_power_iter``, and the sigma it leaves
    is the one the forward's planes are divided by, so the exact-f32 forward has the model's bytes) and divides
    ``weight_bar`` by sigma = u . (W_bar v), through which the gradient does flow.

        z1 = (conv1(X; W_bar / sigma) - mean1) rsqrt(var1 + eps),  zd = (conv_d(X) + bias_d - mean_d) rsqrt(var_d + eps)

    on X = cat(nearest_upsample_2x(x0), x1): what ``V2ce3d.forward_dec2_normed`` returns, with a ``grad_fn``.

    The launches are those ``forward_dec2_inputs`` makes for this block: conv1's and the shortcut's own 1x1x1 launch (in
    ``f16x2`` the model's default path folds the shortcut into conv2's K loop instead).  In ``f16x2`` conv1 is the single
    phase-folded launch on planes of ``W_bar / sigma`` packed at every forward (``v2ce_pack_weights_f16x2_up``): the pair of
    a phase-folded partial launch and a Winograd-T launch on the skip channels, which the model makes for the wider
    decoders, needs the transformed skip planes that ``_prepare`` packs once, and is not made here.  The model packs
    ``W_bar`` once and carries 1 / sigma in the epilogue scale, so in ``f16x2`` the forward is within the split-half
    bound of the model's, not byte-equal.

    ``x0`` and ``x1`` get no gradient: a forward on inputs that require one raises.  ``guard`` (``f16x2``) holds the largest
    range-guard bound of the layer's launches."""

    def __init__(self, model=None, bias: bool = True):
        super().__init__()
        self.weight_bar = nn.Parameter(torch.zeros(C, CIN, 3, 3, 3))
        self.short_weight = nn.Parameter(torch.zeros(C, CIN, 1, 1, 1))
        if bias:
            self.short_bias = nn.Parameter(torch.zeros(C))
        else:
            self.register_parameter("short_bias", None)
        self.register_buffer("weight_u", torch.zeros(C))
        self.register_buffer("weight_v", torch.zeros(CIN * TAPS))
        self.register_buffer("bn1_mean", torch.zeros(C))
        self.register_buffer("bn1_var", torch.ones(C))
        self.register_buffer("bnd_mean", torch.zeros(C))
        self.register_buffer("bnd_var", torch.ones(C))
        self.register_buffer("eps", torch.tensor(1e-5))
        self.register_buffer("guard", torch.zeros(1))   # largest split-half range-guard bound of this layer's launches
        self._model = [model]                            # (a list: the model is not a submodule of this layer)
        self._bufs = {}
        self._sigma = self._sn_ws = None

    @staticmethod
    def _block(model):
        if len(model.UNet.decoders) < 2:
            raise ValueError("the model has no decoder in front of the last one")
        return model.UNet.decoders[-2]

    @classmethod
    def from_model(cls, model) -> "Dec2Convs":
        """A layer holding copies of ``model.UNet.decoders[-2]``'s ``conv1.module`` (weight_bar / weight_u / weight_v),
        ``downsample[0]`` (weight, bias) and of the statistics of ``bn1`` and ``downsample[1]``, on their device; its
        forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = cls._block(model)
        inner, short = blk.conv1.module, blk.downsample[0]
        if tuple(inner.weight_bar.shape) != (C, CIN, 3, 3, 3) or tuple(short.weight.shape) != (C, CIN, 1, 1, 1):
            raise ValueError(f"conv1 of the decoder in front of the last one is {tuple(inner.weight_bar.shape)} and its shortcut "
                             f"{tuple(short.weight.shape)}, not [64, 192, 3, 3, 3] and [64, 192, 1, 1, 1]")
        layer = cls(model, bias=short.bias is not None).to(inner.weight_bar.device)
        with torch.no_grad():
            layer.weight_bar.copy_(inner.weight_bar.detach())
            layer.weight_u.copy_(inner.weight_u.detach())
            layer.weight_v.copy_(inner.weight_v.detach())
            layer.short_weight.copy_(short.weight.detach())
            if short.bias is not None:
                layer.short_bias.copy_(short.bias.detach())
            layer.bn1_mean.copy_(blk.bn1.running_mean)
            layer.bn1_var.copy_(blk.bn1.running_var)
            layer.bnd_mean.copy_(blk.downsample[1].running_mean)
            layer.bnd_var.copy_(blk.downsample[1].running_var)
            layer.eps.fill_(BN_EPS)
        return layer

    def _buffers_for(self, model, split, dev):
        """The layer's own packed-weight buffers for the model's launches: (conv1's, the shortcut's), allocated once per
        precision -- split-half planes (with the phase-folded region of the upsampled channels where the model folds them)
        or the exact-f32 kernels' order."""
        key = (split, split and model._upfold(), str(dev))
        if key not in self._bufs:
            if split:
                self._bufs[key] = (model._split_buffer(C, CIN, TAPS, dev, up_c0=C0 if model._upfold() else 0),
                                   model._split_buffer(C, CIN, 1, dev))
            else:
                self._bufs[key] = (torch.empty(C * CIN * TAPS, dtype=torch.float32, device=dev),
                                   torch.empty(C * CIN, dtype=torch.float32, device=dev))
        return self._bufs[key]

    def effective(self):
        """-> conv1's weight W_bar / sigma as a differentiable tensor, after one power iteration on u / v
        (spectral_norm.py:19-31) by ``v2ce_sn_power_iter``, which also leaves the sigma the forward's planes are divided by
        in ``_sigma``."""
        dev = self.weight_bar.device
        rows, cols = C, CIN * TAPS
        with torch.no_grad(), torch.cuda.device(dev):
            if self._sigma is None or self._sigma.device != dev:
                self._sigma = torch.empty(1, dtype=torch.float32, device=dev)
                self._sn_ws = torch.empty(max(hip.lib().v2ce_sn_workspace_bytes(rows, cols), 16), dtype=torch.uint8, device=dev)
            hip.check(hip.lib().v2ce_sn_power_iter(self.weight_u.data_ptr(), self.weight_v.data_ptr(),
                                                   self.weight_bar.data_ptr(), rows, cols, self._sigma.data_ptr(),
                                                   self._sn_ws.data_ptr(), self._sn_ws.numel(), hip.stream_ptr(dev)),
                      "v2ce_sn_power_iter")
        sigma = self.weight_u.dot(self.weight_bar.view(C, -1).mv(self.weight_v))
        return self.weight_bar / sigma

    def forward(self, x0: torch.Tensor, x1: torch.Tensor):
        """x0 [B, L, 8, H00, pitch00, 16], x1 [B, L, 4, H0, pitch0, 16] (``V2ce3d.forward_dec2_sources``'s h1 and s2) ->
        (z1, zd), the pair ``Dec2Norms`` takes, channels-last-16 [B, L, 4, H0, pitch', 16] with ``.lw`` and a ``grad_fn``."""
        model = self._model[0]
        if model is None:
            raise ValueError("Dec2Convs needs the model whose convolution path it launches: Dec2Convs.from_model(model)")
        c0, c1, _, _, _, W, _, _ = _check_sources(x0, x1)
        if (c0, c1) != (C0, C1):
            raise ValueError(f"x0 must have 128 channels and x1 64, got {tuple(x0.shape)} and {tuple(x1.shape)}")
        if x0.requires_grad or x1.requires_grad:
            raise ValueError("Dec2Convs provides no gradient with respect to x0 and x1 (the input gradient of conv1 and of the "
                             "shortcut through the upsample, a convup_dgrad at 192 -> 64, is not implemented): pass tensors "
                             "that do not require grad")
        if not self.weight_bar.is_contiguous() or self.weight_bar.dtype != torch.float32:
            raise ValueError("weight_bar must be a contiguous float32 tensor")
        z1, zd = _Dec2ConvsFn.apply(x0, x1, self.effective(), self.short_weight, self.short_bias, self)
        for z in (z1, zd):
            z.lw, z.c16 = W, True
        return z1, zd

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and the shortcut's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layers."""
        blk = self._block(model)
        inner, short = blk.conv1.module, blk.downsample[0]
        inner.weight_bar.copy_(self.weight_bar.detach())
        inner.weight_u.copy_(self.weight_u)
        inner.weight_v.copy_(self.weight_v)
        short.weight.copy_(self.short_weight.detach())
        if self.short_bias is not None and short.bias is not None:
            short.bias.copy_(self.short_bias.detach())
        model._prep = None


class Dec2Norms(nn.Module):
    """The affine parts of ``UNet.decoders[2]``'s ``bn1`` (behind conv1) and ``downsample.1`` (on the shortcut) as a
    trainable module on the pair ``V2ce3d.forward_dec2_normed`` returns: ``TailNorms`` (last_conv.py) at 64 channels.

        t2, res2 = norms(z1, zd)                      # relu(w1 z1 + b1), wd zd + bd: what Dec2Conv takes

    The statistics stay frozen (the layer in ``.eval()``).  The forward and its per-channel gradient sums are torch
    expressions over the columns ``[..., :lw, :]`` only: the padding columns of ``z1`` / ``zd`` are uninitialised and never
    enter a sum; those of the returned tensors are zeros.  ``t2`` carries ``.absmax``, the range slot a producing launch
    would have left."""

    def __init__(self):
        super().__init__()
        self.bn1_weight = nn.Parameter(torch.ones(C))
        self.bn1_bias = nn.Parameter(torch.zeros(C))
        self.bnd_weight = nn.Parameter(torch.ones(C))
        self.bnd_bias = nn.Parameter(torch.zeros(C))

    @staticmethod
    def _norms(model):
        blk = Dec2Convs._block(model)
        return blk.bn1, blk.downsample[1]

    @classmethod
    def from_model(cls, model) -> "Dec2Norms":
        """A module holding copies of the affine parameters of ``model.UNet.decoders[-2]``'s ``bn1`` and
        ``downsample[1]``, on their device."""
        bn1, bnd = cls._norms(model)
        if tuple(bn1.weight.shape) != (C,) or tuple(bnd.weight.shape) != (C,):
            raise ValueError(f"the decoder in front of the last one has {tuple(bn1.weight.shape)} channels, not [64]")
        layer = cls().to(bn1.weight.device)
        with torch.no_grad():
            layer.bn1_weight.copy_(bn1.weight.detach())
            layer.bn1_bias.copy_(bn1.bias.detach())
            layer.bnd_weight.copy_(bnd.weight.detach())
            layer.bnd_bias.copy_(bnd.bias.detach())
        return layer

    def forward(self, z1: torch.Tensor, zd: torch.Tensor):
        """z1, zd: channels-last-16 [B, L, 4, H0, pitch0, 16] (``V2ce3d.forward_dec2_normed``) -> (t2, res2) in the same
        layout with ``.lw``, zeros in the padding columns and a ``grad_fn``."""
        dims = _check_c16(z1, "z1", (C,))
        if _check_c16(zd, "zd", (C,)) != dims or zd.shape != z1.shape or zd.device != z1.device:
            raise ValueError(f"zd {tuple(zd.shape)} must match z1 {tuple(z1.shape)}")
        lw, pitch = dims[4], dims[5]
        per = lambda p: p.view(C // 16, 1, 1, 16)            # channel g * 16 + j of [B, L, g, H, column, j]
        t = torch.relu(per(self.bn1_weight) * z1[..., :lw, :] + per(self.bn1_bias))
        res = per(self.bnd_weight) * zd[..., :lw, :] + per(self.bnd_bias)
        t, res = (nn.functional.pad(a, (0, 0, 0, pitch - lw)).contiguous() for a in (t, res))
        for a in (t, res):
            a.lw, a.c16 = lw, True
        # the range slot of the split-half path: [max |t|, no range-guard value] per batch element, what a producing launch
        # would have left (the padding columns are zeros), so conv2 scales t as it does behind forward_dec2_inputs
        amax = t.detach().abs().amax(dim=(1, 2, 3, 4, 5))
        t.absmax = torch.stack([amax, torch.zeros_like(amax)], dim=1).contiguous()
        return t, res

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy the four vectors into ``model`` and drop its derived constants: the next inference call runs the tuned
        BatchNorms."""
        bn1, bnd = self._norms(model)
        bn1.weight.copy_(self.bn1_weight.detach())
        bn1.bias.copy_(self.bn1_bias.detach())
        bnd.weight.copy_(self.bnd_weight.detach())
        bnd.bias.copy_(self.bnd_bias.detach())
        model._prep = None


class Dec2Block(nn.Module):
    """The reference's whole third decoder block ``ResidualBlock3D(192, 64, norm='BN', sn=True)`` on
    ``cat(nearest_upsample_2x(x0), x1)`` as one layer: ``Dec2Convs -> Dec2Norms -> Dec2Conv``, in ``.eval()`` (frozen
    BatchNorm statistics), differentiable in its ten parameter tensors.

        dec2 = Dec2Block.from_model(model)
        x0_last = dec2(h1, s2)                        # the source ``LastBlock`` upsamples, with ``.absmax`` and a grad_fn
        ... .backward()                               # dec2.convs / .norms / .conv parameters
        dec2.write_back(model)

    The two sources get no gradient (``Dec2Convs``)."""

    def __init__(self, convs: Dec2Convs, norms: Dec2Norms, conv: Dec2Conv):
        super().__init__()
        self.convs, self.norms, self.conv = convs, norms, conv

    @classmethod
    def from_model(cls, model) -> "Dec2Block":
        return cls(Dec2Convs.from_model(model), Dec2Norms.from_model(model), Dec2Conv.from_model(model))

    def forward(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """x0 [B, L, 8, H00, pitch00, 16], x1 [B, L, 4, H0, pitch0, 16] (``V2ce3d.forward_dec2_sources``'s h1 and s2) -> the
        block's output [B, L, 4, H0, pitch', 16], what ``Dec2Conv`` returns: ``LastBlock``'s x0 with ``.lw``, ``.absmax``
        (``f16x2``) and a ``grad_fn``."""
        return self.conv(*self.norms(*self.convs(x0, x1)))

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy the three layers' tensors into ``model``: the next inference call runs the tuned block."""
        for m in (self.convs, self.norms, self.conv):
            m.write_back(model)
