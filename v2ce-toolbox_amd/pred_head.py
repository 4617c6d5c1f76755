"""The prediction head ``UNet.pred`` as a trainable layer on the GPU (include/v2ce_hip_train.h, csrc/pred_head.hip).

In the reference it is ``ConvLayer3D(32, 20, 1, activation='relu', norm=None)``: a 1x1x1 convolution with bias followed
by ``torch.relu`` (train/scripts/model/unet_2layer.py:364, submodules.py:79-118).  ``V2ce3d.forward`` runs it fused into
the last decoder convolution, without gradient; here it is a layer of its own on the features
``V2ce3d.forward_features`` returns, with a backward:

    feat = model.forward_features(x)              # the frozen trunk, no gradient
    head = PredHead.from_model(model)             # weight [20, 32, 1, 1, 1], bias [20], requires_grad
    pred = head(feat)                             # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # head.weight.grad, head.bias.grad
    head.write_back(model)                        # the next model(x) runs the tuned head

Tensors: ``feat`` is channels-last-16, ``[B, L, 2, H, pitch, 16]`` f32 with its logical width in ``.lw`` (pitch when the
attribute is missing); ``y`` and ``upstream`` are ``[B, L, Cout, H, W]``.  Every sum is f64 from the f32 inputs and is
rounded once; there are no atomics, so results are identical from run to run.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip

CIN = 32
MAX_COUT = 32
WANT = ("weight", "bias", "feat")


def _overlaps(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * 4 and b0 < a0 + a.numel() * 4


def _check_f32(t, name, device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor (got {type(t)})")
    if not t.is_cuda:
        raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"{name} lives on {t.device}, feat on {device}")


def _check_c16(t, name, channels):
    """-> (C, B, L, H, W, pitch) of a channels-last-16 tensor whose channel count is one of ``channels``: the one shape
    check of the head, the gradient entries (conv_grads.py) and the trainable layers (decoder_block.py)."""
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


def _check_feat(feat, name="feat"):
    """-> (B, L, H, W, pitch) of a channels-last-16 feature tensor."""
    return _check_c16(feat, name, (CIN,))[1:]


def _check_weight(weight, device):
    _check_f32(weight, "weight", device)
    if weight.dim() not in (2, 5) or weight.shape[1] != CIN or weight.numel() != weight.shape[0] * CIN:
        raise ValueError(f"weight must be [cout, 32] or [cout, 32, 1, 1, 1], got {tuple(weight.shape)}")
    cout = int(weight.shape[0])
    if not 1 <= cout <= MAX_COUT:
        raise ValueError(f"weight has {cout} output channels, the head kernels take 1 .. {MAX_COUT}")
    return cout


def _check_dense(t, name, shape, device):
    _check_f32(t, name, device)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be [b, l, cout, h, w] = {list(shape)}, got {tuple(t.shape)}")


def _no_overlap(outs, ins):
    outs = [(n, t) for n, t in outs if t is not None]
    for i, (n, t) in enumerate(outs):
        for m, u in ins:
            if _overlaps(t, u):
                raise ValueError(f"{n} overlaps {m}")
        for m, u in outs[i + 1:]:
            if _overlaps(t, u):
                raise ValueError(f"{n} overlaps {m}")


def pred_head_forward(feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu(conv1x1x1(feat, weight) + bias) -> [B, L, Cout, H, W] f32, every element written; no gradient is recorded
    (``PredHead`` is the differentiable form).  ``out``: write here instead of allocating."""
    B, L, H, W, pitch = _check_feat(feat)
    dev = feat.device
    cout = _check_weight(weight, dev)
    _check_f32(bias, "bias", dev)
    if tuple(bias.shape) != (cout,):
        raise ValueError(f"bias must be [{cout}], got {tuple(bias.shape)}")
    shape = (B, L, cout, H, W)
    if out is not None:
        _check_dense(out, "out", shape, dev)
        _no_overlap([("out", out)], [("feat", feat), ("weight", weight), ("bias", bias)])
    lib = hip.lib()
    nb = lib.v2ce_pred_head_fwd_workspace_bytes(B, L, cout, H, W, pitch)
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_pred_head_fwd: unsupported shape {shape} (pitch {pitch})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        y = torch.empty(shape, dtype=torch.float32, device=dev) if out is None else out
        hip.check(lib.v2ce_pred_head_fwd(feat.data_ptr(), weight.data_ptr(), bias.data_ptr(), B, L, cout, H, W, pitch,
                                         y.data_ptr(), ws.data_ptr(), nb, hip.stream_ptr(dev)), "v2ce_pred_head_fwd")
    return y


def pred_head_grads(feat: torch.Tensor, y: torch.Tensor, upstream: torch.Tensor, weight: torch.Tensor, *,
                    want: Sequence[str] = ("weight", "bias"), out: Optional[dict] = None) -> dict:
    """The backward of ``pred_head_forward``: ``y`` is the forward's output, ``upstream`` the gradient with respect to
    it.  -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'bias', 'feat'; only those are computed):
    'weight' shaped like ``weight``, 'bias' [Cout], 'feat' channels-last-16 with the pitch and ``.lw`` of ``feat`` (its
    padding columns are not written and hold zeros in a tensor allocated here).  ``out``: {name: tensor} to write into
    instead of allocating.  One call, no host synchronisation."""
    want = tuple(want)
    if not want or any(n not in WANT for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {WANT}, got {want}")
    B, L, H, W, pitch = _check_feat(feat)
    dev = feat.device
    cout = _check_weight(weight, dev)
    shape = (B, L, cout, H, W)
    _check_dense(y, "y", shape, dev)
    _check_dense(upstream, "upstream", shape, dev)
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    ins = [("feat", feat), ("y", y), ("upstream", upstream), ("weight", weight)]
    for n, t in out.items():
        if n == "feat":
            _check_f32(t, "out['feat']", dev)
            if t.shape != feat.shape or t.data_ptr() % 16:
                raise ValueError(f"out['feat'] must be 16-byte aligned and shaped like feat {tuple(feat.shape)}, got "
                                 f"{tuple(t.shape)}")
        else:
            _check_f32(t, f"out['{n}']", dev)
            if t.numel() != (cout * CIN if n == "weight" else cout):
                raise ValueError(f"out['{n}'] has {t.numel()} elements")
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    lib = hip.lib()
    nb = lib.v2ce_pred_head_grads_workspace_bytes(B, L, cout, H, W, pitch)
    if nb == 0:
        raise hip.V2ceHipError(f"v2ce_pred_head_grads: unsupported shape {shape} (pitch {pitch})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {}
        for n in want:
            if n in out:
                res[n] = out[n]
            elif n == "weight":
                res[n] = torch.empty_like(weight)
            elif n == "bias":
                res[n] = torch.empty(cout, dtype=torch.float32, device=dev)
            else:
                res[n] = torch.zeros_like(feat) if pitch != W else torch.empty_like(feat)
                res[n].lw, res[n].c16 = W, True
        hip.check(lib.v2ce_pred_head_grads(feat.data_ptr(), y.data_ptr(), upstream.data_ptr(), weight.data_ptr(), B, L, cout,
                                           H, W, pitch, hip.ptr(res.get("weight")), hip.ptr(res.get("bias")),
                                           hip.ptr(res.get("feat")), ws.data_ptr(), nb, hip.stream_ptr(dev)),
                  "v2ce_pred_head_grads")
    return res


class _PredHeadFn(torch.autograd.Function):
    """forward: the forward kernel; backward: one gradient call for the inputs that need a gradient."""

    @staticmethod
    def forward(ctx, feat, weight, bias):
        y = pred_head_forward(feat, weight.detach(), bias.detach())
        ctx.save_for_backward(feat, weight, y)
        ctx.lw = getattr(feat, "lw", None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        feat, weight, y = ctx.saved_tensors
        want = tuple(n for n, need in zip(("feat", "weight", "bias"), ctx.needs_input_grad) if need)
        if not want:
            return None, None, None
        if ctx.lw is not None:                          # (attributes do not survive save_for_backward on every version)
            feat.lw = ctx.lw
        g = pred_head_grads(feat, y, grad_output.contiguous(), weight.detach(), want=want)
        return g.get("feat"), g.get("weight"), g.get("bias")


class PredHead(nn.Module):
    """``UNet.pred`` as a trainable module: ``weight`` [Cout, 32, 1, 1, 1] and ``bias`` [Cout], named and shaped as
    ``UNet.pred.conv3d``'s, both ``requires_grad``.  ``forward(feat)`` takes the channels-last-16 features of
    ``V2ce3d.forward_features`` and returns [B, L, Cout, H, W] with a ``grad_fn``."""

    def __init__(self, out_channels: int = 20):
        super().__init__()
        if not 1 <= int(out_channels) <= MAX_COUT:
            raise ValueError(f"out_channels must be 1 .. {MAX_COUT}, got {out_channels}")
        self.weight = nn.Parameter(torch.zeros(int(out_channels), CIN, 1, 1, 1))
        self.bias = nn.Parameter(torch.zeros(int(out_channels)))

    @classmethod
    def from_model(cls, model) -> "PredHead":
        """A head holding copies of ``model.UNet.pred.conv3d``'s weight and bias, on their device."""
        conv = model.UNet.pred.conv3d
        head = cls(conv.weight.shape[0]).to(conv.weight.device)
        with torch.no_grad():
            head.weight.copy_(conv.weight.detach().reshape(head.weight.shape))
            head.bias.copy_(conv.bias.detach())
        return head

    def forward(self, feat: torch.Tensor) -> torch.Tensor:
        return _PredHeadFn.apply(feat, self.weight, self.bias)

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy both tensors into ``model.UNet.pred.conv3d`` and drop the model's derived constants: the next inference
        call packs the tuned head."""
        conv = model.UNet.pred.conv3d
        conv.weight.copy_(self.weight.detach().reshape(conv.weight.shape))
        conv.bias.copy_(self.bias.detach())
        model._prep = None
