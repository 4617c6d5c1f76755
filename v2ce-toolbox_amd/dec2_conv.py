"""The second convolution of the third decoder block, ``UNet.decoders[2].conv2``, as a trainable layer on the GPU, and the
gradients of a 3x3x3 convolution with 32 or 64 channels on either side that it stands on (include/v2ce_hip_convngrad.h,
csrc/convnwgrad.hip, csrc/convndgrad.hip): the checked entries ``convn_wgrad`` and ``convn_dgrad``.

In the reference the layer is the second convolution of ``ResidualBlock3D(192, 64, norm='BN', sn=True)``: a
spectral-normalised 3x3x3 ``Conv3d(64, 64)`` followed by ``bn2``, the shortcut add and ``relu``
(train/scripts/model/submodules.py:249-264), at half the output resolution.  Its output is ``x0``, the source the last
decoder block upsamples, and ``LastBlock`` (last_block.py) returns ``d_x0``:

    t2, res2, x1 = model.forward_dec2_inputs(x)   # the frozen trunk up to dec2.conv2's two inputs and dec3's skip tensor
    conv = Dec2Conv.from_model(model)             # weight_bar [64, 64, 3, 3, 3], bn_weight [64], bn_bias [64]
    block, head = LastBlock.from_model(model), PredHead.from_model(model)
    pred = head(block(conv(t2, res2), x1))        # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # conv.weight_bar.grad, conv.bn_weight.grad, conv.bn_bias.grad, block.*, head.*
    for m in (conv, block, head): m.write_back(model)

The channel counts of the two entries are read from the tensors: a channels-last-16 tensor with C channels has C / 16
planes, ``[B, L, C / 16, H, pitch, 16]`` f32, and the weight is ``[cout, cin, 3, 3, 3]``; 32 -> 32 restates
``conv32_wgrad`` / ``conv32_dgrad`` (last_conv.py) byte for byte.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .last_conv import _planar_pitched
from .pred_head import _check_f32, _no_overlap

C = 64                     # channels of dec2.conv2 on either side

TAPS = 27
WANT = ("weight", "shift")
DGRAD_WANT = ("x", "res")


def _check_act(t, name):
    """-> (C, B, L, H, W, pitch) of a channels-last-16 tensor with 32 or 64 channels."""
    _check_f32(t, name)
    if t.dim() != 6 or t.shape[5] != 16 or int(t.shape[2]) * 16 not in hip.CONVN_CHANNELS:
        raise ValueError(f"{name} must be channels-last-16 [b, l, 2 or 4, h, pitch, 16], got {tuple(getattr(t, 'shape', ()))}")
    B, L, G, H, pitch, _ = (int(v) for v in t.shape)
    W = int(getattr(t, "lw", pitch))
    if not 1 <= W <= pitch:
        raise ValueError(f"{name}.lw = {W} is outside 1 .. pitch = {pitch}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return G * 16, B, L, H, W, pitch


def _check_pair(y, upstream, dev=None):
    """upstream and (unless None) y: the same shape, ``.lw`` and device -> (cout, B, L, H, W, pitch), [(name, tensor)]."""
    dims = _check_act(upstream, "upstream")
    dev = upstream.device if dev is None else dev
    if upstream.device != dev:
        raise ValueError(f"upstream lives on {upstream.device}, x on {dev}")
    ins = [("upstream", upstream)]
    if y is not None:
        if _check_act(y, "y") != dims or tuple(y.shape) != tuple(upstream.shape):
            raise ValueError(f"y {tuple(y.shape)} (lw {getattr(y, 'lw', y.shape[4])}) must match upstream "
                             f"{tuple(upstream.shape)} (lw {dims[4]})")
        if y.device != dev:
            raise ValueError(f"y lives on {y.device}, upstream on {dev}")
        ins.append(("y", y))
    return dims, ins


def convn_wgrad(x: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = ("weight", "shift"), out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu behind it.
    ``x`` (the convolution's input, cin channels), ``y`` (the relu's output, or None: no mask) and ``upstream`` (the
    gradient with respect to ``y``; both cout channels) are channels-last-16 f32 with the same B, L, H, pitch and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'shift'): 'weight' [cout, cin, 3, 3, 3] = sum over
    the positions of m[co] x[ci] shifted by the tap, 'shift' [cout] = sum of m[co], with m = upstream where y > 0 else 0.
    ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the shares of the
    tile walk at max(n / pairs, 1), pairs = (cout / 32) (cin / 32) (the result then depends on n only through the order
    of the f64 sums).  One call, no host synchronisation."""
    want = tuple(want)
    if not want or any(n not in WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    cin, B, L, H, W, pitch = _check_act(x, "x")
    dev = x.device
    (cout, *pos), ins = _check_pair(y, upstream, dev)
    if tuple(pos) != (B, L, H, W, pitch):
        raise ValueError(f"upstream {tuple(upstream.shape)} (lw {pos[3]}) must match x {tuple(x.shape)} (lw {W}) but for the planes")
    ins.append(("x", x))
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if t.numel() != (cout * cin * TAPS if n == "weight" else cout):
            raise ValueError(f"out['{n}'] has {t.numel()} elements")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_convn_wgrad_workspace_bytes(cin, cout, B, L, H, W, pitch, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_convn_wgrad: unsupported shape {(B, L, H, W)} (pitch {pitch}, {cin} -> {cout})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {}
        for n in want:
            if n in out:
                res[n] = out[n]
            elif n == "weight":
                res[n] = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=dev)
            else:
                res[n] = torch.empty(cout, dtype=torch.float32, device=dev)
        hip.check(lib.v2ce_convn_wgrad(x.data_ptr(), hip.ptr(y), upstream.data_ptr(), cin, cout, B, L, H, W, pitch,
                                       hip.ptr(res.get("weight")), hip.ptr(res.get("shift")), ws.data_ptr(), nb,
                                       int(max_workgroups), hip.stream_ptr(dev)), "v2ce_convn_wgrad")
    return res


def convn_dgrad(weight: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = ("x", "res"), out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The input gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu behind it.
    ``weight`` is the convolution's own contiguous ``[cout, cin, 3, 3, 3]`` f32 weight; ``y`` (the relu's output, or None:
    no mask) and ``upstream`` (the gradient with respect to ``y``) are channels-last-16 f32 with cout channels, the same
    shape and ``.lw``.  -> {name: tensor} for the names in ``want`` (a subset of 'x', 'res'): 'x' (cin channels) = the
    transposed convolution of m with the weight, 'res' (cout channels) = m, with m = upstream where y > 0 else 0; both
    carry upstream's pitch and ``.lw`` and zeros in the padding columns ``lw .. pitch - 1``.  ``out``: {name: tensor} to
    write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the grid (the bytes do not depend on n).  One
    call, no host synchronisation."""
    want = tuple(want)
    if not want or any(n not in DGRAD_WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {DGRAD_WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    (cout, B, L, H, W, pitch), ins = _check_pair(y, upstream)
    dev = upstream.device
    _check_f32(weight, "weight", dev)
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or int(weight.shape[0]) != cout or \
            int(weight.shape[1]) not in hip.CONVN_CHANNELS:
        raise ValueError(f"weight must be [{cout}, 32 or 64, 3, 3, 3] (upstream has {cout} channels), got {tuple(weight.shape)}")
    cin = int(weight.shape[1])
    ins.append(("weight", weight))
    shapes = {"x": (B, L, cin // 16, H, pitch, 16), "res": tuple(upstream.shape)}
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if tuple(t.shape) != shapes[n]:
            raise ValueError(f"out['{n}'] {tuple(t.shape)} must be {shapes[n]}")
        if t.data_ptr() % 16:
            raise ValueError(f"out['{n}'] must be 16-byte aligned")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_convn_dgrad_workspace_bytes(cin, cout, B, L, H, W, pitch, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_convn_dgrad: unsupported shape {(B, L, H, W)} (pitch {pitch}, {cin} -> {cout})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {n: out[n] if n in out else torch.empty(shapes[n], dtype=torch.float32, device=dev) for n in want}
        hip.check(lib.v2ce_convn_dgrad(weight.data_ptr(), hip.ptr(y), upstream.data_ptr(), cin, cout, B, L, H, W, pitch,
                                       hip.ptr(res.get("x")), hip.ptr(res.get("res")), ws.data_ptr(), nb,
                                       int(max_workgroups), hip.stream_ptr(dev)), "v2ce_convn_dgrad")
    for t in res.values():
        t.lw, t.c16 = W, True
    return res


class _Dec2ConvFn(torch.autograd.Function):
    """forward: x0 = relu(scale * conv(t, W_bar / sigma) + shift + res) as one launch of the model's convolution path, on
    planes packed from W_bar and the sigma of the layer's power iteration as the model packs its own; backward: one
    v2ce_convn_wgrad call with the layer's own output as y (the relu's mask), then dW = scale dM, d_scale = <W, dM>,
    d_shift; and, when t or res requires grad, one v2ce_convn_dgrad call on the weight with bn2's scale folded in
    (scale[co] W[co], 110 592 products in torch: one more rounding per term) for d_t and d_res = the masked upstream.

    ``.c16`` / ``.lw``: as for ``_LastConvFn``, a returned gradient has the layout, the pitch and the logical width of the
    tensor it belongs to, and its padding columns are zeros."""

    @staticmethod
    def forward(ctx, t, res, W, scale, shift, layer):
        model = layer._model[0]
        split = model.precision == "f16x2"
        with torch.no_grad(), torch.cuda.device(t.device):
            if model._prep is None:
                model._prepare()
            P = model._prep
            Wd = W.detach().contiguous()
            packed = model._pack(layer.weight_bar.detach().contiguous(), layer._sigma, split=split)
            sc, sh = scale.detach().contiguous(), shift.detach().contiguous()
            # the launch takes its range slot from the model's table: a table of this call's own, put back afterwards
            saved = (P["absmax"], getattr(model, "_slot", 0))
            P["absmax"], model._slot = torch.zeros((1, t.shape[0], 2), dtype=torch.float32, device=t.device), 0
            try:
                if split:
                    feat = model._conv(t, None, packed, sc, sh, C, 3, 1, hip.ACT_RELU, residual=res, split=True, track=True)
                    torch.maximum(layer.guard, feat.absmax[:, 1].max().reshape(1), out=layer.guard)
                    layer._slot_out = feat.absmax        # this call's table: the range slot of the layer's output
                    del feat.absmax
                else:
                    y = model._conv(_planar_pitched(t), None, packed, sc, sh, C, 3, 1, hip.ACT_RELU,
                                    residual=_planar_pitched(res), split=False)
                    feat = model.to_c16(y)
                    layer._slot_out = None
            finally:
                P["absmax"], model._slot = saved
        ctx.save_for_backward(t, feat, Wd, sc)
        ctx.lw = getattr(t, "lw", t.shape[4])
        feat.lw, feat.c16 = ctx.lw, True
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        t, feat, W, scale = ctx.saved_tensors
        need_t, need_res, need_w, need_scale, need_shift = ctx.needs_input_grad[:5]
        if not (need_t or need_res or need_w or need_scale or need_shift):
            return (None,) * 6
        t.lw = feat.lw = ctx.lw                         # (attributes do not survive save_for_backward on every version)
        g = grad_output.contiguous()
        g.lw = ctx.lw
        dW = d_scale = d_shift = d_t = d_res = None
        want = (("weight",) if need_w or need_scale else ()) + (("shift",) if need_shift else ())
        if want:
            r = convn_wgrad(t, feat, g, want=want)
            dM = r.get("weight")
            dW = scale.view(C, 1, 1, 1, 1) * dM if need_w else None
            d_scale = (W * dM).sum(dim=(1, 2, 3, 4)) if need_scale else None
            d_shift = r.get("shift")
        want = (("x",) if need_t else ()) + (("res",) if need_res else ())
        if want:
            r = convn_dgrad((scale.view(C, 1, 1, 1, 1) * W).contiguous(), feat, g, want=want)
            d_t, d_res = r.get("x"), r.get("res")
        return d_t, d_res, dW, d_scale, d_shift, None


class Dec2Conv(nn.Module):
    """``UNet.decoders[2].conv2`` + ``bn2`` + shortcut add + relu as a trainable module, the layer in ``.eval()``: the
    BatchNorm statistics are frozen, its affine parameters and the convolution's ``weight_bar`` train.  Like the
    reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` / ``weight_v`` by one power iteration (no
    gradient; the model's own kernel, so the exact-f32 forward has the model's bytes) and divides ``weight_bar`` by sigma =
    u . (W_bar v), through which the gradient does flow.  ``t`` and ``res`` receive gradients when they require grad
    (``v2ce_convn_dgrad``: one more launch, none otherwise); like every channels-last-16 gradient they have ``t``'s pitch
    and ``.lw`` and zeros in the padding columns.

    The output is ``x0``, the source of the last decoder block (``LastBlock``), with a ``grad_fn``: the relu that
    ``LastBlock`` leaves to the consumer of ``d_x0`` is this layer's own, and its mask is taken from the layer's output.

    Range slot (``f16x2``): the output carries ``.absmax`` -- max |x0| per batch element, what the model's launch leaves
    -- so the block behind scales it as it does behind ``forward_tail_sources``; a ``t`` without ``.absmax`` runs on the
    kernel's fixed pre-scale.  ``guard`` holds the largest range-guard bound of the layer's launches."""

    def __init__(self, model=None):
        super().__init__()
        self.weight_bar = nn.Parameter(torch.zeros(C, C, 3, 3, 3))
        self.bn_weight = nn.Parameter(torch.ones(C))
        self.bn_bias = nn.Parameter(torch.zeros(C))
        self.register_buffer("weight_u", torch.zeros(C))
        self.register_buffer("weight_v", torch.zeros(C * TAPS))
        self.register_buffer("running_mean", torch.zeros(C))
        self.register_buffer("running_var", torch.ones(C))
        self.register_buffer("eps", torch.tensor(1e-5))
        self.register_buffer("guard", torch.zeros(1))   # largest split-half range-guard bound of this layer's launches
        self._model = [model]                            # (a list: the model is not a submodule of this layer)
        self._sigma = self._sn_ws = self._slot_out = None

    @staticmethod
    def _block(model):
        if len(model.UNet.decoders) < 2:
            raise ValueError("the model has no decoder in front of the last one")
        return model.UNet.decoders[-2]

    @classmethod
    def from_model(cls, model) -> "Dec2Conv":
        """A layer holding copies of ``model.UNet.decoders[-2].conv2.module``'s weight_bar / weight_u / weight_v and of
        ``.bn2``'s tensors, on their device; its forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = cls._block(model)
        inner, bn = blk.conv2.module, blk.bn2
        if tuple(inner.weight_bar.shape) != (C, C, 3, 3, 3):
            raise ValueError(f"the convolution in front of the last decoder block is {tuple(inner.weight_bar.shape)}, not "
                             f"[64, 64, 3, 3, 3]")
        layer = cls(model).to(inner.weight_bar.device)
        with torch.no_grad():
            layer.weight_bar.copy_(inner.weight_bar.detach())
            layer.weight_u.copy_(inner.weight_u.detach())
            layer.weight_v.copy_(inner.weight_v.detach())
            layer.bn_weight.copy_(bn.weight.detach())
            layer.bn_bias.copy_(bn.bias.detach())
            layer.running_mean.copy_(bn.running_mean)
            layer.running_var.copy_(bn.running_var)
            layer.eps.fill_(BN_EPS)
        return layer

    def effective(self):
        """-> (W, scale, shift) as differentiable tensors, after one power iteration on u / v (spectral_norm.py:19-31) by
        ``v2ce_sn_power_iter``, which also leaves the sigma the forward's planes are divided by in ``_sigma``.  scale and
        shift are formed as the model folds a BatchNorm (``V2ce3d._fold_bn``)."""
        dev = self.weight_bar.device
        rows, cols = C, C * TAPS
        with torch.no_grad(), torch.cuda.device(dev):
            if self._sigma is None or self._sigma.device != dev:
                self._sigma = torch.empty(1, dtype=torch.float32, device=dev)
                self._sn_ws = torch.empty(max(hip.lib().v2ce_sn_workspace_bytes(rows, cols), 16), dtype=torch.uint8, device=dev)
            hip.check(hip.lib().v2ce_sn_power_iter(self.weight_u.data_ptr(), self.weight_v.data_ptr(),
                                                   self.weight_bar.data_ptr(), rows, cols, self._sigma.data_ptr(),
                                                   self._sn_ws.data_ptr(), self._sn_ws.numel(), hip.stream_ptr(dev)),
                      "v2ce_sn_power_iter")
        sigma = self.weight_u.dot(self.weight_bar.view(C, -1).mv(self.weight_v))
        W = self.weight_bar / sigma
        scale = self.bn_weight / torch.sqrt(self.running_var + self.eps)
        shift = self.bn_bias - self.running_mean * scale
        return W, scale, shift

    def forward(self, t: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
        """t, res: channels-last-16 [B, L, 4, H0, pitch0, 16] (``V2ce3d.forward_dec2_inputs``) -> the block's output x0 in the
        same layout, what ``LastBlock`` takes as its first input, with a ``grad_fn``."""
        model = self._model[0]
        if model is None:
            raise ValueError("Dec2Conv needs the model whose convolution path it launches: Dec2Conv.from_model(model)")
        dims = _check_act(t, "t")
        if dims[0] != C:
            raise ValueError(f"t must have 64 channels [b, l, 4, h0, pitch0, 16], got {tuple(t.shape)}")
        if _check_act(res, "res") != dims or res.shape != t.shape or res.device != t.device:
            raise ValueError(f"res {tuple(res.shape)} must match t {tuple(t.shape)}")
        if not self.weight_bar.is_contiguous() or self.weight_bar.dtype != torch.float32:
            raise ValueError("weight_bar must be a contiguous float32 tensor")
        W, scale, shift = self.effective()
        feat = _Dec2ConvFn.apply(t, res, W, scale, shift, self)
        feat.lw, feat.c16 = dims[4], True
        if self._slot_out is not None:
            feat.absmax, self._slot_out = self._slot_out, None
        return feat

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and bn2's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layer."""
        blk = self._block(model)
        inner, bn = blk.conv2.module, blk.bn2
        inner.weight_bar.copy_(self.weight_bar.detach())
        inner.weight_u.copy_(self.weight_u)
        inner.weight_v.copy_(self.weight_v)
        bn.weight.copy_(self.bn_weight.detach())
        bn.bias.copy_(self.bn_bias.detach())
        model._prep = None
