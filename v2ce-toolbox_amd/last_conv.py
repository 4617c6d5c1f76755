"""The last decoder convolution ``UNet.decoders[3].conv2`` as a trainable layer on the GPU (include/v2ce_hip_convgrad.h,
csrc/convnwgrad.hip; include/v2ce_hip_convdgrad.h, csrc/convndgrad.hip).

In the reference it is the second convolution of ``ResidualBlock3D(96, 32, norm='BN', sn=True)``: a spectral-normalised
3x3x3 ``Conv3d(32, 32)`` followed by ``bn2``, the shortcut add and ``relu`` (train/scripts/model/submodules.py:210-258,
spectral_norm.py:19-31).  ``V2ce3d.forward`` runs it without gradient; here it is a layer of its own on the two tensors
``V2ce3d.forward_tail_inputs`` returns, with a backward for its parameters:

    t, res = model.forward_tail_inputs(x)         # the frozen trunk up to conv2's input, no gradient
    conv = LastConv.from_model(model)             # weight_bar [32, 32, 3, 3, 3], bn_weight [32], bn_bias [32]
    head = PredHead.from_model(model)
    pred = head(conv(t, res))                     # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # conv.weight_bar.grad, conv.bn_weight.grad, conv.bn_bias.grad, head.*
    conv.write_back(model); head.write_back(model)

The forward is the model's own convolution launch at the model's precision; the backward is one ``v2ce_conv32_wgrad``
call (exact-f32 MFMA products in chains of at most ``hip.WGRAD_CHAIN`` positions, f64 above, no atomics: identical bytes
from run to run) and a few 32 x 864 torch expressions.  When ``t`` or ``res`` requires grad, the backward also makes one
``v2ce_conv32_dgrad`` call (exact-f32 MFMA, ``hip.DGRAD_TERMS`` f32 terms per element in a fixed order, no atomics) and
returns the gradients with respect to both: that is what lets a layer in front of this one train (``TailNorms``).  With
neither requiring grad nothing more is launched.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .pred_head import _check_f32, _check_feat, _no_overlap

C = 32
TAPS = 27
WANT = ("weight", "shift")
DGRAD_WANT = ("x", "res")


def conv32_wgrad(x: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                 want: Sequence[str] = ("weight", "shift"), out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradient of a stride-1, zero-padded 3x3x3 convolution 32 -> 32 seen through the relu behind it.
    ``x`` (the convolution's input), ``y`` (the relu's output, or None: no mask) and ``upstream`` (the gradient with
    respect to ``y``) are channels-last-16 ``[B, L, 2, H, pitch, 16]`` f32 with the same shape and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'shift'): 'weight' [32, 32, 3, 3, 3] = sum over
    the positions of m[co] x[ci] shifted by the tap, 'shift' [32] = sum of m[co], with m = upstream where y > 0 else 0.
    ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the grid (the result
    then depends on n only through the order of the f64 sums).  One call, no host synchronisation."""
    want = tuple(want)
    if not want or any(n not in WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    B, L, H, W, pitch = _check_feat(x, "x")
    dev = x.device
    ins = [("x", x)]
    for n, t in (("y", y), ("upstream", upstream)):
        if t is None and n == "y":
            continue
        dims = _check_feat(t, n)
        if t.device != dev:
            raise ValueError(f"{n} lives on {t.device}, x on {dev}")
        if tuple(t.shape) != tuple(x.shape) or dims != (B, L, H, W, pitch):
            raise ValueError(f"{n} {tuple(t.shape)} (lw {dims[3]}) must match x {tuple(x.shape)} (lw {W})")
        ins.append((n, t))
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if t.numel() != (C * C * TAPS if n == "weight" else C):
            raise ValueError(f"out['{n}'] has {t.numel()} elements")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_conv32_wgrad_workspace_bytes(B, L, H, W, pitch, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_conv32_wgrad: unsupported shape {(B, L, H, W)} (pitch {pitch})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {}
        for n in want:
            if n in out:
                res[n] = out[n]
            elif n == "weight":
                res[n] = torch.empty((C, C, 3, 3, 3), dtype=torch.float32, device=dev)
            else:
                res[n] = torch.empty(C, dtype=torch.float32, device=dev)
        hip.check(lib.v2ce_conv32_wgrad(x.data_ptr(), hip.ptr(y), upstream.data_ptr(), B, L, H, W, pitch,
                                        hip.ptr(res.get("weight")), hip.ptr(res.get("shift")), ws.data_ptr(), nb,
                                        int(max_workgroups), hip.stream_ptr(dev)), "v2ce_conv32_wgrad")
    return res


def conv32_dgrad(weight: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                 want: Sequence[str] = ("x", "res"), out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The input gradient of a stride-1, zero-padded 3x3x3 convolution 32 -> 32 seen through the relu behind it.
    ``weight`` is the convolution's own contiguous ``[32, 32, 3, 3, 3]`` f32 weight; ``y`` (the relu's output, or None: no
    mask) and ``upstream`` (the gradient with respect to ``y``) are channels-last-16 ``[B, L, 2, H, pitch, 16]`` f32 with
    the same shape and ``.lw``.  -> {name: tensor} for the names in ``want`` (a subset of 'x', 'res'), both in the layout
    of ``upstream`` with its ``.lw``: 'x' = the transposed convolution of m with the weight, 'res' = m, with m = upstream
    where y > 0 else 0.  Their padding columns ``lw .. pitch - 1`` are zeros.  ``out``: {name: tensor} to write into.
    ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the grid (the bytes do not depend on n).  One call, no host
    synchronisation."""
    want = tuple(want)
    if not want or any(n not in DGRAD_WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {DGRAD_WANT}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    B, L, H, W, pitch = _check_feat(upstream, "upstream")
    dev = upstream.device
    ins = [("upstream", upstream)]
    if y is not None:
        dims = _check_feat(y, "y")
        if y.device != dev:
            raise ValueError(f"y lives on {y.device}, upstream on {dev}")
        if tuple(y.shape) != tuple(upstream.shape) or dims != (B, L, H, W, pitch):
            raise ValueError(f"y {tuple(y.shape)} (lw {dims[3]}) must match upstream {tuple(upstream.shape)} (lw {W})")
        ins.append(("y", y))
    _check_f32(weight, "weight", dev)
    if tuple(weight.shape) != (C, C, 3, 3, 3):
        raise ValueError(f"weight must be [32, 32, 3, 3, 3], got {tuple(weight.shape)}")
    ins.append(("weight", weight))
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        if tuple(t.shape) != tuple(upstream.shape):
            raise ValueError(f"out['{n}'] {tuple(t.shape)} must match upstream {tuple(upstream.shape)}")
        if t.data_ptr() % 16:
            raise ValueError(f"out['{n}'] must be 16-byte aligned")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_conv32_dgrad_workspace_bytes(B, L, H, W, pitch, int(max_workgroups))
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_conv32_dgrad: unsupported shape {(B, L, H, W)} (pitch {pitch})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {n: out[n] if n in out else torch.empty_like(upstream) for n in want}
        hip.check(lib.v2ce_conv32_dgrad(weight.data_ptr(), hip.ptr(y), upstream.data_ptr(), B, L, H, W, pitch,
                                        hip.ptr(res.get("x")), hip.ptr(res.get("res")), ws.data_ptr(), nb,
                                        int(max_workgroups), hip.stream_ptr(dev)), "v2ce_conv32_dgrad")
    for t in res.values():
        t.lw, t.c16 = W, True
    return res


def _planar_pitched(x: torch.Tensor) -> torch.Tensor:
    """Channels-last-16 -> planar [B, T, C, H, pitch] with the padding columns kept (what the exact-f32 launches take as a
    residual: its pitch is the output's)."""
    B, T, G, H, Wp, _ = x.shape
    y = x.permute(0, 1, 2, 5, 3, 4).reshape(B, T, G * 16, H, Wp).contiguous()
    y.lw = getattr(x, "lw", Wp)
    return y


class _LastConvFn(torch.autograd.Function):
    """forward: feat = relu(scale * conv(t, W) + shift + res) as one launch of the model's convolution path; backward:
    one v2ce_conv32_wgrad call, then dW = scale dM, d_scale = <W, dM>, d_shift; and, when t or res requires grad, one
    v2ce_conv32_dgrad call on the weight with bn2's scale folded in (scale[co] W[co], 27 648 products in torch: one more
    rounding per term) for d_t and d_res = the masked upstream.

    ``.c16`` / ``.lw``: autograd hands the returned gradients on as plain tensors, so ``t.grad`` and ``res.grad`` do not
    carry the attributes.  The convention holds all the same: a gradient has the layout, the pitch and the logical width
    ``.lw`` of the tensor it belongs to, and its padding columns ``lw .. pitch - 1`` are zeros.  ``conv32_dgrad`` sets
    the attributes on the tensors it returns; the package's own consumer, ``TailNorms``, takes the gradient through
    torch's slicing and padding ops over the logical columns and needs neither."""

    @staticmethod
    def forward(ctx, t, res, W, scale, shift, model, guard):
        split = model.precision == "f16x2"
        with torch.no_grad(), torch.cuda.device(t.device):
            if model._prep is None:
                model._prepare()
            P = model._prep
            Wd = W.detach().contiguous()
            packed = model._pack(Wd, split=split)
            sc, sh = scale.detach().contiguous(), shift.detach().contiguous()
            # the launch takes its range slot from the model's table: a table of this call's own, put back afterwards
            saved = (P["absmax"], getattr(model, "_slot", 0))
            P["absmax"], model._slot = torch.zeros((1, t.shape[0], 2), dtype=torch.float32, device=t.device), 0
            try:
                if split:
                    feat = model._conv(t, None, packed, sc, sh, C, 3, 1, hip.ACT_RELU, residual=res, split=True, track=True)
                    torch.maximum(guard, feat.absmax[:, 1].max().reshape(1), out=guard)
                else:
                    y = model._conv(_planar_pitched(t), None, packed, sc, sh, C, 3, 1, hip.ACT_RELU,
                                    residual=_planar_pitched(res), split=False)
                    feat = model.to_c16(y)
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
            return (None,) * 7
        t.lw = feat.lw = ctx.lw                         # (attributes do not survive save_for_backward on every version)
        g = grad_output.contiguous()
        g.lw = ctx.lw
        dW = d_scale = d_shift = d_t = d_res = None
        want = (("weight",) if need_w or need_scale else ()) + (("shift",) if need_shift else ())
        if want:
            r = conv32_wgrad(t, feat, g, want=want)
            dM = r.get("weight")
            dW = scale.view(C, 1, 1, 1, 1) * dM if need_w else None
            d_scale = (W * dM).sum(dim=(1, 2, 3, 4)) if need_scale else None
            d_shift = r.get("shift")
        want = (("x",) if need_t else ()) + (("res",) if need_res else ())
        if want:
            r = conv32_dgrad((scale.view(C, 1, 1, 1, 1) * W).contiguous(), feat, g, want=want)
            d_t, d_res = r.get("x"), r.get("res")
        return d_t, d_res, dW, d_scale, d_shift, None, None


class LastConv(nn.Module):
    """``UNet.decoders[-1].conv2`` + ``bn2`` + shortcut add + relu as a trainable module, the layer in ``.eval()``: the
    BatchNorm statistics are frozen (what a fine-tune on one recording wants), its affine parameters and the
    convolution's ``weight_bar`` train.  Like the reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` /
    ``weight_v`` by one power iteration (no gradient) and divides ``weight_bar`` by sigma = u . (W_bar v), through which
    the gradient does flow.  ``t`` and ``res`` receive gradients when they require grad (``v2ce_conv32_dgrad``: one more
    launch, none otherwise); like every channels-last-16 gradient they have ``t``'s pitch and ``.lw`` and zeros in the
    padding columns.

    Range slot (``f16x2``): a ``t`` without ``.absmax`` -- one that neither ``forward_tail_inputs`` nor ``TailNorms``
    made -- runs on the kernel's fixed pre-scale, and ``guard`` reports the layer's range-guard bound, exactly as for any
    tensor without a range slot.  ``TailNorms`` fills the slot in: max |t| per batch element."""

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

    @classmethod
    def from_model(cls, model) -> "LastConv":
        """A layer holding copies of ``model.UNet.decoders[-1].conv2.module``'s weight_bar / weight_u / weight_v and of
        ``.bn2``'s tensors, on their device; its forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = model.UNet.decoders[-1]
        inner, bn = blk.conv2.module, blk.bn2
        if tuple(inner.weight_bar.shape) != (C, C, 3, 3, 3):
            raise ValueError(f"the last decoder convolution is {tuple(inner.weight_bar.shape)}, not [32, 32, 3, 3, 3]")
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
        """-> (W, scale, shift) as differentiable tensors, after one power iteration on u / v (spectral_norm.py:19-31)."""
        w2 = self.weight_bar.view(C, -1)
        with torch.no_grad():
            wd = w2.detach()
            v = torch.mv(wd.t(), self.weight_u)
            self.weight_v.copy_(v / (v.norm() + 1e-12))
            u = torch.mv(wd, self.weight_v)
            self.weight_u.copy_(u / (u.norm() + 1e-12))
        sigma = self.weight_u.dot(w2.mv(self.weight_v))
        W = self.weight_bar / sigma
        scale = self.bn_weight * torch.rsqrt(self.running_var + self.eps)
        shift = self.bn_bias - self.running_mean * scale
        return W, scale, shift

    def forward(self, t: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
        """t, res: channels-last-16 [B, L, 2, H, pitch, 16] (``V2ce3d.forward_tail_inputs``) -> the block's output, the
        features ``PredHead`` takes, with a ``grad_fn``."""
        model = self._model[0]
        if model is None:
            raise ValueError("LastConv needs the model whose convolution path it launches: LastConv.from_model(model)")
        dims = _check_feat(t, "t")
        if _check_feat(res, "res") != dims or res.shape != t.shape or res.device != t.device:
            raise ValueError(f"res {tuple(res.shape)} must match t {tuple(t.shape)}")
        W, scale, shift = self.effective()
        feat = _LastConvFn.apply(t, res, W, scale, shift, model, self.guard)
        feat.lw, feat.c16 = dims[3], True
        return feat

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and bn2's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layer."""
        blk = model.UNet.decoders[-1]
        inner, bn = blk.conv2.module, blk.bn2
        inner.weight_bar.copy_(self.weight_bar.detach())
        inner.weight_u.copy_(self.weight_u)
        inner.weight_v.copy_(self.weight_v)
        bn.weight.copy_(self.bn_weight.detach())
        bn.bias.copy_(self.bn_bias.detach())
        model._prep = None


class TailNorms(nn.Module):
    """The affine parts of the last decoder block's other two BatchNorms -- ``bn1`` behind conv1 and ``downsample.1`` on
    the shortcut -- as a trainable module on the pair ``V2ce3d.forward_tail_normed`` returns:

        z1, zd = model.forward_tail_normed(x)         # normalised, pre-affine, no gradient
        norms = TailNorms.from_model(model)           # bn1_weight, bn1_bias, bnd_weight, bnd_bias [32]
        t, res = norms(z1, zd)                        # relu(w1 z1 + b1), wd zd + bd: what LastConv takes
        head(conv(t, res)) ... .backward()            # the four gradients pass through conv2 (v2ce_conv32_dgrad)

    The statistics stay frozen (the layer in ``.eval()``).  The forward and its per-channel gradient sums are torch
    expressions over the columns ``[..., :lw, :]`` only: the padding columns of ``z1`` / ``zd`` are uninitialised and
    never enter a sum; those of the returned tensors are zeros."""

    def __init__(self):
        super().__init__()
        self.bn1_weight = nn.Parameter(torch.ones(C))
        self.bn1_bias = nn.Parameter(torch.zeros(C))
        self.bnd_weight = nn.Parameter(torch.ones(C))
        self.bnd_bias = nn.Parameter(torch.zeros(C))

    @staticmethod
    def _norms(model):
        blk = model.UNet.decoders[-1]
        return blk.bn1, blk.downsample[1]

    @classmethod
    def from_model(cls, model) -> "TailNorms":
        """A module holding copies of the affine parameters of ``model.UNet.decoders[-1]``'s ``bn1`` and
        ``downsample[1]``, on their device."""
        bn1, bnd = cls._norms(model)
        if tuple(bn1.weight.shape) != (C,) or tuple(bnd.weight.shape) != (C,):
            raise ValueError(f"the last decoder block has {tuple(bn1.weight.shape)} channels, not [32]")
        layer = cls().to(bn1.weight.device)
        with torch.no_grad():
            layer.bn1_weight.copy_(bn1.weight.detach())
            layer.bn1_bias.copy_(bn1.bias.detach())
            layer.bnd_weight.copy_(bnd.weight.detach())
            layer.bnd_bias.copy_(bnd.bias.detach())
        return layer

    def forward(self, z1: torch.Tensor, zd: torch.Tensor):
        """z1, zd: channels-last-16 [B, L, 2, H, pitch, 16] (``V2ce3d.forward_tail_normed``) -> (t, res) in the same
        layout with ``.lw``, zeros in the padding columns and a ``grad_fn``."""
        dims = _check_feat(z1, "z1")
        if _check_feat(zd, "zd") != dims or zd.shape != z1.shape or zd.device != z1.device:
            raise ValueError(f"zd {tuple(zd.shape)} must match z1 {tuple(z1.shape)}")
        lw, pitch = dims[3], dims[4]
        per = lambda p: p.view(2, 1, 1, 16)                  # channel g * 16 + j of [B, L, g, H, column, j]
        t = torch.relu(per(self.bn1_weight) * z1[..., :lw, :] + per(self.bn1_bias))
        res = per(self.bnd_weight) * zd[..., :lw, :] + per(self.bnd_bias)
        t, res = (nn.functional.pad(a, (0, 0, 0, pitch - lw)).contiguous() for a in (t, res))
        for a in (t, res):
            a.lw, a.c16 = lw, True
        # the range slot of the split-half path: [max |t|, no range-guard value] per batch element, what a producing launch
        # would have left (the padding columns are zeros), so conv2 scales t as it does behind forward_tail_inputs
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
