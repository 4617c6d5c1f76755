"""The first half of the last decoder block -- the spectral-normalised 3x3x3 ``conv1`` and the 1x1x1 shortcut convolution
``downsample.0`` of ``UNet.decoders[3]``, both ``Conv3d(96, 32)`` on ``cat(nearest_upsample_2x(dec2 output), skip)`` -- as
trainable layers on the GPU (include/v2ce_hip_convupgrad.h, csrc/convupnwgrad.hip).

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
32 x 2592 and 32 x 96 results.

The gradients with respect to the two sources are ``convup_dgrad`` (include/v2ce_hip_convupdgrad.h, csrc/convupdgrad.hip):
one ``v2ce_convup_dgrad`` call gives ``d_x1`` and ``d_x0``, the latter pooled back through the 2x nearest upsample, from the
channels-last-16 gradients the block already holds -- neither the concat nor the upsampled tensor is materialised.
``TailConvs(input_grads=True)`` returns them from its backward, and ``LastBlock`` composes the whole block as one layer that
is differentiable in every parameter and in both inputs:

    block = LastBlock.from_model(model)           # TailConvs(input_grads=True) -> TailNorms -> LastConv
    feat = block(x0, x1)                          # x0 / x1 may require grad: x0.grad, x1.grad after backward

``d_x0`` is the gradient with respect to the block's source as the block reads it; a relu in front of it (dec2's) is the
business of whoever consumes the gradient.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .last_conv import LastConv, TailNorms, _planar_pitched
from .pred_head import _check_f32, _check_feat, _no_overlap

C = 32                     # output channels
C0, C1 = 64, 32            # upsampled channels, skip channels
CIN = C0 + C1
TAPS = 27
WANT = ("weight", "short", "short_bias")
_SHAPES = {"weight": (C, CIN, 3, 3, 3), "short": (C, CIN), "short_bias": (C,)}
DGRAD_WANT = ("x0", "x1")


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


def convup_dgrad(weight: Optional[torch.Tensor], short_weight: Optional[torch.Tensor], g1: Optional[torch.Tensor],
                 gd: Optional[torch.Tensor], *, want: Sequence[str] = DGRAD_WANT, out: Optional[dict] = None,
                 max_workgroups: int = 0) -> dict:
    """The gradients of the 3x3x3 and the 1x1x1 convolution 96 -> 32 on the virtual tensor
    ``X = cat(nearest_upsample_2x(x0), x1)`` with respect to ``x0`` and ``x1``.  ``weight`` is the 3x3x3 convolution's own
    contiguous ``[32, 96, 3, 3, 3]`` f32 weight, ``short_weight`` the 1x1x1 convolution's ``[32, 96]`` (or
    ``[32, 96, 1, 1, 1]``); ``g1`` (the gradient with respect to the 3x3x3 convolution's output) and ``gd`` (the gradient
    with respect to the 1x1x1 convolution's output) are channels-last-16 ``[B, L, 2, H, pitch, 16]`` f32 with the same shape
    and ``.lw``.  ``g1`` may be None (``weight`` is then unused): the 1x1x1 convolution's share alone; ``gd`` may be None
    (``short_weight`` likewise); not both.
    -> {name: tensor} for the names in ``want`` (a subset of 'x0', 'x1'): 'x1' ``[B, L, 2, H, pitch, 16]`` = the last 32
    channels of d_X = conv_transpose(g1, weight) + short_weight^T gd, 'x0' ``[B, L, 4, H0, pitch0, 16]`` with
    ``H0 = (H + 1) // 2``, ``.lw = (W + 1) // 2`` and ``pitch0 = V2ce3d._pitch(.lw)`` (or that of ``out['x0']``) = the first
    64 channels summed over the output positions of each source pixel.  Both carry ``.lw`` and ``.c16``; their padding
    columns are zeros.  ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the
    grid (the bytes do not depend on n).  One call, no host synchronisation."""
    from .v2ce_3d import V2ce3d, _nearest_is_half
    want = tuple(want)
    if not want or any(n not in DGRAD_WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {DGRAD_WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    if g1 is None and gd is None:
        raise ValueError("g1 and gd are both None")
    if g1 is not None and weight is None:
        raise ValueError("g1 needs weight")
    if gd is not None and short_weight is None:
        raise ValueError("gd needs short_weight")
    lead, lead_name = (g1, "g1") if g1 is not None else (gd, "gd")
    B, L, H, W, pitch = _check_feat(lead, lead_name)
    dev = lead.device
    ins = [(lead_name, lead)]
    if g1 is not None and gd is not None:
        dims = _check_feat(gd, "gd")
        if gd.device != dev:
            raise ValueError(f"gd lives on {gd.device}, g1 on {dev}")
        if tuple(gd.shape) != tuple(g1.shape) or dims != (B, L, H, W, pitch):
            raise ValueError(f"gd {tuple(gd.shape)} (lw {dims[3]}) must match g1 {tuple(g1.shape)} (lw {W})")
        ins.append(("gd", gd))
    for n, t, shapes, used in (("weight", weight, ((C, CIN, 3, 3, 3),), g1 is not None),
                               ("short_weight", short_weight, ((C, CIN), (C, CIN, 1, 1, 1)), gd is not None)):
        if not used:
            continue
        _check_f32(t, n, dev)
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{n} must be {' or '.join(str(list(s)) for s in shapes)}, got {tuple(t.shape)}")
        ins.append((n, t))
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    if not (_nearest_is_half(H0, H) and _nearest_is_half(W0, W)):
        raise ValueError(f"the nearest upsample {(H0, W0)} -> {(H, W)} does not read its source at (h >> 1, w >> 1)")
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    pitch0 = V2ce3d._pitch(W0)
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if n == "x1" and tuple(t.shape) != tuple(lead.shape):
            raise ValueError(f"out['x1'] {tuple(t.shape)} must match {lead_name} {tuple(lead.shape)}")
        if n == "x0":
            if t.dim() != 6 or tuple(t.shape[:4]) != (B, L, C0 // 16, H0) or t.shape[4] < W0 or t.shape[5] != 16:
                raise ValueError(f"out['x0'] {tuple(t.shape)} must be [{B}, {L}, 4, {H0}, pitch0 >= {W0}, 16]")
            pitch0 = int(t.shape[4])
        if t.data_ptr() % 16:
            raise ValueError(f"out['{n}'] must be 16-byte aligned")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_convup_dgrad_workspace_bytes(B, L, H, W, pitch, pitch0, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_convup_dgrad: unsupported shape {(B, L, H, W)} (pitch {pitch}, pitch0 {pitch0})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        shape = {"x0": (B, L, C0 // 16, H0, pitch0, 16), "x1": tuple(lead.shape)}
        res = {n: out[n] if n in out else torch.empty(shape[n], dtype=torch.float32, device=dev) for n in want}
        hip.check(lib.v2ce_convup_dgrad(hip.ptr(weight) if g1 is not None else None,
                                        hip.ptr(short_weight) if gd is not None else None, hip.ptr(g1), hip.ptr(gd),
                                        B, L, H, W, pitch, pitch0, hip.ptr(res.get("x0")), hip.ptr(res.get("x1")),
                                        ws.data_ptr(), nb, int(max_workgroups), hip.stream_ptr(dev)), "v2ce_convup_dgrad")
    for n, t in res.items():
        t.lw, t.c16 = (W0 if n == "x0" else W), True
    return res


class _TailConvsFn(torch.autograd.Function):
    """forward: z1 = rs1 conv1(X; W) + shift1 and zd = rsd conv_d(X; Wd) + shift_d as the model's own launches on X =
    cat(upsample(x0), x1) -- f16x2: one phase-folded launch with the shortcut fused in, f32: the two unfused launches --
    on weight buffers packed from W and Wd; backward: one v2ce_convup_wgrad call on the gradients of (z1, zd), then
    dW = rs1[co] dM1[co], dWd = rsd[co] dMd[co], d_bias_d = rsd[co] sum gd[co] (the normalisations are per output channel
    and linear, so they commute with the sums over the positions); and, when x0 or x1 requires grad (a layer built with
    ``input_grads=True``), one v2ce_convup_dgrad call on the weights with the normalisations folded in (rs1[co] W[co] and
    rsd[co] Wd[co], 82 944 + 3 072 products in torch: one more rounding per term) for d_x0 and d_x1, only those needed.

    ``.c16`` / ``.lw``: autograd hands the returned gradients on as plain tensors; as for ``_LastConvFn``, a gradient has
    the layout, the pitch and the logical width of the tensor it belongs to, and its padding columns are zeros."""

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
        ctx.save_for_backward(x0, x1, rs1, rsd, Wd, Sd)
        ctx.lw0, ctx.lw = getattr(x0, "lw", x0.shape[4]), up_to[1]
        for z in (z1, zd):
            z.lw, z.c16 = up_to[1], True
        return z1, zd

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, gd):
        x0, x1, rs1, rsd, W, short_w = ctx.saved_tensors
        need_x0, need_x1, need_w, need_sw, need_sb = ctx.needs_input_grad[:5]
        x0.lw, x1.lw = ctx.lw0, ctx.lw                  # (attributes do not survive save_for_backward on every version)
        want = (("weight",) if need_w and g1 is not None else ()) + (("short",) if need_sw and gd is not None else ()) + \
            (("short_bias",) if need_sb and gd is not None else ())
        want_x = (("x0",) if need_x0 else ()) + (("x1",) if need_x1 else ())
        if (g1 is None and gd is None) or not (want or want_x):
            return (None,) * 6
        if g1 is not None:
            g1 = g1.contiguous()
            g1.lw = ctx.lw
        if gd is not None:
            gd = gd.contiguous()
            gd.lw = ctx.lw
        r = convup_wgrad(x0, x1, g1, gd, want=want) if want else {}
        dW = rs1.view(C, 1, 1, 1, 1) * r["weight"] if "weight" in r else None
        d_sw = (rsd.view(C, 1) * r["short"]).view(C, CIN, 1, 1, 1) if "short" in r else None
        d_sb = rsd * r["short_bias"] if "short_bias" in r else None
        d_x0 = d_x1 = None
        if want_x:
            rx = convup_dgrad((rs1.view(C, 1, 1, 1, 1) * W).contiguous() if g1 is not None else None,
                              (rsd.view(C, 1) * short_w.view(C, CIN)).contiguous() if gd is not None else None, g1, gd,
                              want=want_x, out={"x0": torch.empty_like(x0)} if need_x0 else None)
            d_x0, d_x1 = rx.get("x0"), rx.get("x1")
        return d_x0, d_x1, dW, d_sw, d_sb, None


class TailConvs(nn.Module):
    """``UNet.decoders[-1].conv1`` and ``.downsample[0]`` with the normalising halves of ``bn1`` and ``downsample[1]`` as a
    trainable module, the layer in ``.eval()``: the BatchNorm statistics are frozen buffers (their affine parts are
    ``TailNorms``'), conv1's ``weight_bar`` and the shortcut's weight (and bias, where the model has one) train.  Like the
    reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` / ``weight_v`` by one power iteration (no
    gradient) and divides ``weight_bar`` by sigma = u . (W_bar v), through which the gradient does flow.

        z1 = (conv1(X; W_bar / sigma) - mean1) rsqrt(var1 + eps),  zd = (conv_d(X) + bias_d - mean_d) rsqrt(var_d + eps)

    on X = cat(nearest_upsample_2x(x0), x1): what ``V2ce3d.forward_tail_normed`` returns, with a ``grad_fn``.  By default
    ``x0`` and ``x1`` get no gradient: a forward on inputs that require one raises.  With ``input_grads=True`` the forward
    accepts them and the backward returns ``d_x0`` / ``d_x1`` for those that require grad (``convup_dgrad``: one more
    launch, none when neither does; the parameter gradients are the same bytes either way).  ``guard`` (``f16x2``) holds
    the largest range-guard bound of the layer's launches."""

    def __init__(self, model=None, bias: bool = True, input_grads: bool = False):
        super().__init__()
        self.input_grads = bool(input_grads)
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
    def from_model(cls, model, input_grads: bool = False) -> "TailConvs":
        """A layer holding copies of ``model.UNet.decoders[-1]``'s ``conv1.module`` (weight_bar / weight_u / weight_v),
        ``downsample[0]`` (weight, bias) and of the statistics of ``bn1`` and ``downsample[1]``, on their device; its
        forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = model.UNet.decoders[-1]
        inner, short = blk.conv1.module, blk.downsample[0]
        if tuple(inner.weight_bar.shape) != (C, CIN, 3, 3, 3) or tuple(short.weight.shape) != (C, CIN, 1, 1, 1):
            raise ValueError(f"the last decoder block's conv1 is {tuple(inner.weight_bar.shape)} and its shortcut "
                             f"{tuple(short.weight.shape)}, not [32, 96, 3, 3, 3] and [32, 96, 1, 1, 1]")
        layer = cls(model, bias=short.bias is not None, input_grads=input_grads).to(inner.weight_bar.device)
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
        if not self.input_grads and (x0.requires_grad or x1.requires_grad):
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


class LastBlock(nn.Module):
    """The reference's whole last decoder block ``ResidualBlock3D(96, 32, norm='BN', sn=True)`` on
    ``cat(nearest_upsample_2x(x0), x1)`` as one layer: ``TailConvs(input_grads=True) -> TailNorms -> LastConv``, in
    ``.eval()`` (frozen BatchNorm statistics), differentiable in its ten parameter tensors and in both inputs.

        block = LastBlock.from_model(model)
        feat = block(x0, x1)                          # the features ``PredHead`` takes, with a grad_fn
        ... .backward()                               # block.convs / .norms / .conv parameters, x0.grad, x1.grad
        block.write_back(model)

    ``x0.grad`` is the gradient with respect to the block's source as the block reads it, channels-last-16 in ``x0``'s own
    shape with zeros in the padding columns; the relu of the decoder in front (``x0 > 0``) is not applied."""

    def __init__(self, convs: TailConvs, norms: TailNorms, conv: LastConv):
        super().__init__()
        self.convs, self.norms, self.conv = convs, norms, conv

    @classmethod
    def from_model(cls, model) -> "LastBlock":
        return cls(TailConvs.from_model(model, input_grads=True), TailNorms.from_model(model), LastConv.from_model(model))

    def forward(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """x0 [B, L, 4, H0, pitch0, 16], x1 [B, L, 2, H, pitch, 16] (``V2ce3d.forward_tail_sources``, or tensors of the
        caller's own that require grad) -> the block's output [B, L, 2, H, pitch', 16] with ``.lw`` and a ``grad_fn``."""
        return self.conv(*self.norms(*self.convs(x0, x1)))

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy the three layers' tensors into ``model``: the next inference call runs the tuned block."""
        for m in (self.convs, self.norms, self.conv):
            m.write_back(model)
