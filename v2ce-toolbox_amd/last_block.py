"""The first half of the last decoder block -- the spectral-normalised 3x3x3 ``conv1`` and the 1x1x1 shortcut convolution
``downsample.0`` of ``UNet.decoders[3]``, both ``Conv3d(96, 32)`` on ``cat(nearest_upsample_2x(dec2 output), skip)`` -- as
trainable layers on the GPU (include/v2ce_hip_convupgrad.h, csrc/convupgrad.hip).

    x0, x1 = model.forward_tail_sources(x)        # the frozen trunk up to the block's two sources, no gradient
    convs = TailConvs.from_model(model)           # weight_bar [32, 96, 3, 3, 3], short_weight [32, 96, 1, 1, 1], short_bias
    norms, conv, head = TailNorms.from_model(model), LastConv.from_model(model), PredHead.from_model(model)
    pred = head(conv(*norms(*convs(x0, x1))))     # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # convs.weight_bar.grad, convs.short_weight.grad, ... and the layers' behind
    for m in (convs, norms, conv, head): m.write_back(model)

With ``TailNorms`` and ``LastConv`` this is the reference's whole ``ResidualBlock3D(96, 32, norm='BN', sn=True)``.  The
forward is the model's own convolution launch at the model's precision; the backward is one ``v2ce_convup_wgrad`` call
(exact-f32 MFMA products in chains of at most ``hip.UPWGRAD_CHAIN`` positions, f64 above, no atomics: identical bytes from
run to run) that reads the upsampled channels at ``(h >> 1, w >> 1)`` of their source, and a few torch expressions on its
32 x 2592 and 32 x 96 results.  The gradients with respect to ``x0`` and ``x1`` are not provided.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .last_conv import _planar_pitched
from .pred_head import _check_f32, _check_feat, _no_overlap

C = 32                     # output channels
C0, C1 = 64, 32            # upsampled channels, skip channels
CIN = C0 + C1
TAPS = 27
WANT = ("weight", "short", "short_bias")
_SHAPES = {"weight": (C, CIN, 3, 3, 3), "short": (C, CIN), "short_bias": (C,)}


def _check_src(x0, name="x0"):
    """-> (B, L, H0, W0, pitch0) of the channels-last-16 source of the upsampled channels, [b, l, 4, h0, pitch0, 16]."""
    _check_f32(x0, name)
    if x0.dim() != 6 or x0.shape[2] != C0 // 16 or x0.shape[5] != 16:
        raise ValueError(f"{name} must be channels-last-16 [b, l, 4, h0, pitch0, 16], got {tuple(getattr(x0, 'shape', ()))}")
    B, L, _, H0, pitch0, _ = (int(v) for v in x0.shape)
    W0 = int(getattr(x0, "lw", pitch0))
    if not 1 <= W0 <= pitch0:
        raise ValueError(f"{name}.lw = {W0} is outside 1 .. pitch0 = {pitch0}")
    if x0.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return B, L, H0, W0, pitch0


def convup_wgrad(x0: torch.Tensor, x1: torch.Tensor, g1: Optional[torch.Tensor], gd: Optional[torch.Tensor], *,
                 want: Sequence[str] = WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradients of the 3x3x3 and the 1x1x1 convolution 96 -> 32 on the virtual tensor
    ``X = cat(nearest_upsample_2x(x0), x1)``.  ``x0`` is channels-last-16 ``[B, L, 4, H0, pitch0, 16]`` f32 with
    ``H0 = (H + 1) // 2`` and ``.lw = (W + 1) // 2``; ``x1`` (the skip tensor), ``g1`` (the gradient with respect to the
    3x3x3 convolution's output) and ``gd`` (the gradient with respect to the 1x1x1 convolution's output) are
    channels-last-16 ``[B, L, 2, H, pitch, 16]`` f32 with the same shape and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'short', 'short_bias'): 'weight' [32, 96, 3, 3, 3] =
    sum over the positions of g1[co] X[ci] shifted by the tap (zero padding at the upsampled resolution), 'short' [32, 96] =
    sum of gd[co] X[ci], 'short_bias' [32] = sum of gd[co].  ``g1`` may be None without 'weight', ``gd`` without 'short'
    and 'short_bias'.  ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the
    grid (the result then depends on n only through the order of the f64 sums).  One call, no host synchronisation."""
    from .v2ce_3d import _nearest_is_half
    want = tuple(want)
    if not want or any(n not in WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    if "weight" in want and g1 is None:
        raise ValueError("want 'weight' needs g1")
    if ("short" in want or "short_bias" in want) and gd is None:
        raise ValueError("want 'short' and 'short_bias' need gd")
    B, L, H, W, pitch = _check_feat(x1, "x1")
    dev = x1.device
    B0, L0, H0, W0, pitch0 = _check_src(x0)
    if x0.device != dev:
        raise ValueError(f"x0 lives on {x0.device}, x1 on {dev}")
    if (B0, L0) != (B, L) or H0 != (H + 1) // 2 or W0 != (W + 1) // 2:
        raise ValueError(f"x0 {tuple(x0.shape)} (lw {W0}) must match x1 {tuple(x1.shape)} (lw {W}): the same b and l, "
                         f"h0 = (h + 1) // 2 = {(H + 1) // 2} and lw = {(W + 1) // 2}")
    if not (_nearest_is_half(H0, H) and _nearest_is_half(W0, W)):
        raise ValueError(f"the nearest upsample {(H0, W0)} -> {(H, W)} does not read its source at (h >> 1, w >> 1)")
    ins = [("x0", x0), ("x1", x1)]
    for n, t in (("g1", g1), ("gd", gd)):
        if t is None:
            continue
        dims = _check_feat(t, n)
        if t.device != dev:
            raise ValueError(f"{n} lives on {t.device}, x1 on {dev}")
        if tuple(t.shape) != tuple(x1.shape) or dims != (B, L, H, W, pitch):
            raise ValueError(f"{n} {tuple(t.shape)} (lw {dims[3]}) must match x1 {tuple(x1.shape)} (lw {W})")
        ins.append((n, t))
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if t.numel() != torch.Size(_SHAPES[n]).numel():
            raise ValueError(f"out['{n}'] has {t.numel()} elements")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_convup_wgrad_workspace_bytes(B, L, H, W, pitch, pitch0, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_convup_wgrad: unsupported shape {(B, L, H, W)} (pitch {pitch}, pitch0 {pitch0})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {n: out[n] if n in out else torch.empty(_SHAPES[n], dtype=torch.float32, device=dev) for n in want}
        hip.check(lib.v2ce_convup_wgrad(x0.data_ptr(), x1.data_ptr(), hip.ptr(g1) if "weight" in want else None,
                                        hip.ptr(gd) if ("short" in want or "short_bias" in want) else None,
                                        B, L, H, W, pitch, pitch0, hip.ptr(res.get("weight")), hip.ptr(res.get("short")),
                                        hip.ptr(res.get("short_bias")), ws.data_ptr(), nb, int(max_workgroups),
                                        hip.stream_ptr(dev)), "v2ce_convup_wgrad")
    return res


class _TailConvsFn(torch.autograd.Function):
    """forward: z1 = rs1 conv1(X; W) + shift1 and zd = rsd conv_d(X; Wd) + shift_d as the model's own launches on X =
    cat(upsample(x0), x1) -- f16x2: one phase-folded launch with the shortcut fused in, f32: the two unfused launches --
    on weight buffers packed from W and Wd; backward: one v2ce_convup_wgrad call on the gradients of (z1, zd), then
    dW = rs1[co] dM1[co], dWd = rsd[co] dMd[co], d_bias_d = rsd[co] sum gd[co] (the normalisations are per output channel
    and linear, so they commute with the sums over the positions)."""

    @staticmethod
    def forward(ctx, x0, x1, W, short_w, short_b, layer):
        model = layer._model[0]
        split = model.precision == "f16x2"
        blk = model.UNet.decoders[-1]
        dev = x1.device
        with torch.no_grad(), torch.cuda.device(dev):
            if model._prep is None:
                model._prepare()
            P = model._prep
            rs1 = (1.0 / torch.sqrt(layer.bn1_var + layer.eps)).float().contiguous()
            rsd = (1.0 / torch.sqrt(layer.bnd_var + layer.eps)).float().contiguous()
            shift1 = (-layer.bn1_mean * rs1).float().contiguous()
            shift_d = (-layer.bnd_mean * rsd if short_b is None else (short_b.detach() - layer.bnd_mean) * rsd).float().contiguous()
            Wd, Sd = W.detach().contiguous(), short_w.detach().contiguous()
            w1, wd = layer._buffers_for(model, split, dev)
            model._pack(Wd, None, w1, split=split)
            model._pack(Sd, None, wd, split=split)
            up_to = (int(x1.shape[3]), int(getattr(x1, "lw", x1.shape[4])))
            # the launches take their range slot from the model's table: a table of this call's own, put back afterwards
            saved = (P["absmax"], getattr(model, "_slot", 0))
            P["absmax"], model._slot = torch.zeros((2, x1.shape[0], 2), dtype=torch.float32, device=dev), 0
            try:
                if split:
                    assert model._fuse_shortcut(blk), "the 32-channel block's shortcut rides on conv1's launch"
                    z1, zd = model._conv(x0, x1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=True,
                                         sc=(wd, rsd, shift_d))
                    torch.maximum(layer.guard, z1.absmax[:, 1].max().reshape(1), out=layer.guard)
                    del z1.absmax                       # (a view of this call's table)
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
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise RuntimeError("TailConvs provides no gradient with respect to x0 and x1 (the input gradients of conv1 and "
                               "of the shortcut are not implemented)")
        need_w, need_sw, need_sb = ctx.needs_input_grad[2:5]
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
        r = convup_wgrad(x0, x1, g1, gd, want=want)
        dW = rs1.view(C, 1, 1, 1, 1) * r["weight"] if "weight" in r else None
        d_sw = (rsd.view(C, 1) * r["short"]).view(C, CIN, 1, 1, 1) if "short" in r else None
        d_sb = rsd * r["short_bias"] if "short_bias" in r else None
        return None, None, dW, d_sw, d_sb, None


class TailConvs(nn.Module):
    """``UNet.decoders[-1].conv1`` and ``.downsample[0]`` with the normalising halves of ``bn1`` and ``downsample[1]`` as a
    trainable module, the layer in ``.eval()``: the BatchNorm statistics are frozen buffers (their affine parts are
    ``TailNorms``'), conv1's ``weight_bar`` and the shortcut's weight (and bias, where the model has one) train.  Like the
    reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` / ``weight_v`` by one power iteration (no
    gradient) and divides ``weight_bar`` by sigma = u . (W_bar v), through which the gradient does flow.

        z1 = (conv1(X; W_bar / sigma) - mean1) rsqrt(var1 + eps),  zd = (conv_d(X) + bias_d - mean_d) rsqrt(var_d + eps)

    on X = cat(nearest_upsample_2x(x0), x1): what ``V2ce3d.forward_tail_normed`` returns, with a ``grad_fn``.  ``x0`` and
    ``x1`` get no gradient: a forward on inputs that require one raises.  ``guard`` (``f16x2``) holds the largest
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

    @classmethod
    def from_model(cls, model) -> "TailConvs":
        """A layer holding copies of ``model.UNet.decoders[-1]``'s ``conv1.module`` (weight_bar / weight_u / weight_v),
        ``downsample[0]`` (weight, bias) and of the statistics of ``bn1`` and ``downsample[1]``, on their device; its
        forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = model.UNet.decoders[-1]
        inner, short = blk.conv1.module, blk.downsample[0]
        if tuple(inner.weight_bar.shape) != (C, CIN, 3, 3, 3) or tuple(short.weight.shape) != (C, CIN, 1, 1, 1):
            raise ValueError(f"the last decoder block's conv1 is {tuple(inner.weight_bar.shape)} and its shortcut "
                             f"{tuple(short.weight.shape)}, not [32, 96, 3, 3, 3] and [32, 96, 1, 1, 1]")
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
        (spectral_norm.py:19-31)."""
        w2 = self.weight_bar.view(C, -1)
        with torch.no_grad():
            wd = w2.detach()
            v = torch.mv(wd.t(), self.weight_u)
            self.weight_v.copy_(v / (v.norm() + 1e-12))
            u = torch.mv(wd, self.weight_v)
            self.weight_u.copy_(u / (u.norm() + 1e-12))
        sigma = self.weight_u.dot(w2.mv(self.weight_v))
        return self.weight_bar / sigma

    def forward(self, x0: torch.Tensor, x1: torch.Tensor):
        """x0 [B, L, 4, H0, pitch0, 16], x1 [B, L, 2, H, pitch, 16] (``V2ce3d.forward_tail_sources``) -> (z1, zd), the pair
        ``TailNorms`` takes, channels-last-16 [B, L, 2, H, pitch', 16] with ``.lw`` and a ``grad_fn``."""
        from .v2ce_3d import _nearest_is_half
        model = self._model[0]
        if model is None:
            raise ValueError("TailConvs needs the model whose convolution path it launches: TailConvs.from_model(model)")
        B, L, H, W, _ = _check_feat(x1, "x1")
        B0, L0, H0, W0, _ = _check_src(x0)
        if (B0, L0) != (B, L) or H0 != (H + 1) // 2 or W0 != (W + 1) // 2 or x0.device != x1.device:
            raise ValueError(f"x0 {tuple(x0.shape)} (lw {W0}) must match x1 {tuple(x1.shape)} (lw {W}): the same b and l, "
                             f"h0 = (h + 1) // 2 and lw = (w + 1) // 2")
        if not (_nearest_is_half(H0, H) and _nearest_is_half(W0, W)):
            raise ValueError(f"the nearest upsample {(H0, W0)} -> {(H, W)} does not read its source at (h >> 1, w >> 1)")
        if x0.requires_grad or x1.requires_grad:
            raise ValueError("TailConvs provides no gradient with respect to x0 and x1 (the input gradients of conv1 and of "
                             "the shortcut are not implemented): pass tensors that do not require grad")
        z1, zd = _TailConvsFn.apply(x0, x1, self.effective(), self.short_weight, self.short_bias, self)
        for z in (z1, zd):
            z.lw, z.c16 = W, True
        return z1, zd

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and the shortcut's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layers."""
        blk = model.UNet.decoders[-1]
        inner, short = blk.conv1.module, blk.downsample[0]
        inner.weight_bar.copy_(self.weight_bar.detach())
        inner.weight_u.copy_(self.weight_u)
        inner.weight_v.copy_(self.weight_v)
        short.weight.copy_(self.short_weight.detach())
        if self.short_bias is not None and short.bias is not None:
            short.bias.copy_(self.short_bias.detach())
        model._prep = None
