"""Fit the prediction head to a recording: the smallest training workflow of the reference (everything frozen but
``UNet.pred`` in train/main.py), entirely on the package's own kernels.

    history = fit_head(model, image_units, gt_voxels, steps=200, lr=1e-3)

The trunk is frozen, so its output -- the 32-channel features in front of ``UNet.pred`` -- is computed once per window
(``V2ce3d.forward_features``) and every step is ``PredHead`` -> ``losses.calculate_loss`` -> ``backward()`` -> one
``torch.optim`` step on the head's 660 parameters.  The deeper fits (``fit_tail`` ... ``fit_dec1_conv``) train one more
layer each; ``STAGES`` lists them and ``_fit`` is the loop they share.  ``v2ce_finetune.py`` is the command line (``main``
below).
"""
from __future__ import annotations

import argparse
import importlib
import json
import logging
import os
import os.path as op
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import losses
from .pred_head import PredHead

logger = logging.getLogger("V2CE")
DEFAULT_CACHE_BYTES = 8 << 30


def _windows(image_units, gt_voxels):
    """-> [(x [B, L, 2, H, W], gt [B, L, 20, H, W])]: the model calls of one pass over the data."""
    xs = list(image_units) if isinstance(image_units, (list, tuple)) else [image_units]
    gs = list(gt_voxels) if isinstance(gt_voxels, (list, tuple)) else [gt_voxels]
    if len(xs) != len(gs) or not xs:
        raise ValueError(f"{len(xs)} image-unit windows for {len(gs)} ground-truth windows")
    for x, g in zip(xs, gs):
        if not (isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor)) or x.dim() != 5 or g.dim() != 5:
            raise ValueError("every window is a pair of tensors [b, l, 2, h, w] and [b, l, 20, h, w]")
        if (x.shape[0], x.shape[1], x.shape[3], x.shape[4]) != (g.shape[0], g.shape[1], g.shape[3], g.shape[4]):
            raise ValueError(f"image units {tuple(x.shape)} and ground truth {tuple(g.shape)} differ in b, l, h or w")
    return list(zip(xs, gs))


class Stage(NamedTuple):
    """One training depth.  ``groups``: the parameter groups the stage adds to the shallower ones', each {name: (role,
    attributes)} (an attribute that is None on the layer, a shortcut without bias, is left out).  ``accessor``: the
    ``V2ce3d`` method whose tensors a fit of this depth caches.  ``layers``: every layer behind the cached tensors but the
    head, shallowest first, as (role, "module.Class"); a ``DecoderBlock`` of role r fills the roles r.convs, r.norms and
    r.conv.  The layers are built and written back in this order and chained in the reverse one: each takes the first
    two tensors of the list (the cached ones at first) and puts its output, one tensor or a pair, in their place; the
    head takes the one that is left."""
    name: str
    choice: str                 # the command line's --train value
    groups: dict
    accessor: str
    layers: tuple


_LAST = (("last.conv", "last_conv.LastConv"), ("last.norms", "last_conv.TailNorms"), ("last.convs", "last_block.TailConvs"))
_BLOCK = ("last", "last_block.LastBlock")
_CONV2 = lambda role: (role, ("weight_bar",))
_BN = lambda role, bn="bn": (role, (bn + "_weight", bn + "_bias"))
_SHORT = lambda role: (role, ("short_weight", "short_bias"))

STAGES = (
    Stage("head", "head", {"pred": ("head", ("weight", "bias"))}, "forward_features", ()),
    Stage("tail", "tail", {"conv2": _CONV2("last.conv"), "bn2": _BN("last.conv")}, "forward_tail_inputs", _LAST[:1]),
    Stage("tail_norms", "tail_norms", {"bn1": _BN("last.norms", "bn1"), "bnd": _BN("last.norms", "bnd")},
          "forward_tail_normed", _LAST[:2]),
    Stage("last_block", "last_block", {"conv1": _CONV2("last.convs"), "convd": _SHORT("last.convs")},
          "forward_tail_sources", _LAST),
    Stage("dec2_conv", "dec2_conv2", {"dec2_conv2": _CONV2("dec2.conv"), "dec2_bn2": _BN("dec2.conv")},
          "forward_dec2_inputs", (_BLOCK, ("dec2.conv", "dec2_conv.Dec2Conv"))),
    Stage("dec2_block", "dec2_block",
          {"dec2_conv1": _CONV2("dec2.convs"), "dec2_convd": _SHORT("dec2.convs"), "dec2_bn1": _BN("dec2.norms", "bn1"),
           "dec2_bnd": _BN("dec2.norms", "bnd")},
          "forward_dec2_sources", (_BLOCK, ("dec2", "dec2_block.Dec2Block"))),
    Stage("dec1_conv", "dec1_conv2", {"dec1_conv2": _CONV2("dec1.conv"), "dec1_bn2": _BN("dec1.conv")},
          "forward_dec1_inputs", (_BLOCK, ("dec2", "dec2_block.Dec2BlockThrough"), ("dec1.conv", "dec1_conv.Dec1Conv"))),
)


def _depth(train, allowed) -> int:
    """-> the index in ``STAGES`` of the deepest stage that has a group in ``train``: the depth to which layers are built.
    ``train`` must be a non-empty subset of ``allowed`` without repeats."""
    train = tuple(train)
    if not train or any(g not in allowed for g in train) or len(set(train)) != len(train):
        raise ValueError(f"train must be a non-empty subset of {allowed}, got {train}")
    return max(i for i, stage in enumerate(STAGES) if any(g in stage.groups for g in train))


def _build(model, stage):
    """-> (the stage's layers in the order of ``stage.layers``, {role: layer} with the head's)."""
    from .decoder_block import DecoderBlock
    head = PredHead.from_model(model)
    layers, roles = [], {"head": head}
    for role, path in stage.layers:
        module, cls = path.split(".")
        layer = getattr(importlib.import_module("." + module, __package__), cls).from_model(model)
        layers.append(layer)
        if isinstance(layer, DecoderBlock):
            roles.update({f"{role}.convs": layer.convs, f"{role}.norms": layer.norms, f"{role}.conv": layer.conv})
        else:
            roles[role] = layer
    return head, layers, roles


def _fit(model, image_units, gt_voxels, *, allowed, train, loss, steps, lr, optimizer, cache_bytes, loss_options) -> List[dict]:
    """The loop of every ``fit_*``: train the groups ``train`` (a subset of ``allowed``) at the depth of the deepest one.

    The tensors of the depth's accessor are computed once per window and kept while the kept ones fit in ``cache_bytes``; a
    window beyond the budget is recomputed at each of its steps.  Every such pass starts from the spectral-norm state the
    model had on entry, so a window's tensors do not depend on whether they were cached.  Every step is the depth's layers
    -> ``PredHead`` -> ``losses.calculate_loss`` -> ``backward()`` -> one optimizer step on the parameters of ``train``, in
    its order; every group of the depth has ``requires_grad`` set, to whether it is trained.  On return the model's
    spectral-norm u / v and call counter are restored, then every layer built writes its tensors back.
    (``loss_options`` is a dict, not ``**``: a stray keyword of a caller stays a loss option.)"""
    depth = _depth(train, allowed)
    train = tuple(train)
    loss = losses.check_loss_names(loss)
    if optimizer not in ("adam", "sgd"):
        raise ValueError(f"optimizer must be 'adam' or 'sgd', got {optimizer!r}")
    if int(steps) < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    windows = _windows(image_units, gt_voxels)
    stage = STAGES[depth]
    head, layers, roles = _build(model, stage)
    groups = {g: [p for p in (getattr(roles[role], a) for a in attrs) if p is not None]
              for s in STAGES[:depth + 1] for g, (role, attrs) in s.groups.items()}
    for g, ps in groups.items():
        for p in ps:
            p.requires_grad_(g in train)
    opt = (torch.optim.Adam if optimizer == "adam" else torch.optim.SGD)([p for g in train for p in groups[g]], lr=lr)
    snap = model.sn_snapshot()
    cache, used = {}, 0

    def inputs(i):
        nonlocal used
        if i in cache:
            return cache[i]
        model.sn_restore(snap)
        out = getattr(model, stage.accessor)(windows[i][0])
        out = out if isinstance(out, tuple) else (out,)
        nb = sum(a.numel() for a in out) * 4
        if used + nb <= cache_bytes:
            cache[i], used = out, used + nb
        return out

    history = []
    try:
        for k in range(int(steps)):
            i = k % len(windows)
            opt.zero_grad(set_to_none=True)
            args = list(inputs(i))
            for layer in reversed(layers):
                out = layer(args[0], args[1])
                args[:2] = out if isinstance(out, tuple) else (out,)
            pred = head(*args)
            total, d = losses.calculate_loss(pred, windows[i][1].contiguous(), loss=loss, **loss_options)
            total.backward()
            opt.step()
            history.append({"loss": float(total.detach()), "loss_dict": {n: float(v) for n, v in d.items()}})
    finally:
        model.sn_restore(snap)
    guards = [float(layer.guard) for layer in roles.values() if hasattr(layer, "guard")]
    if guards and model.precision == "f16x2" and max(guards) > model.RANGE_GUARD_LIMIT:
        logger.warning(f"split-half range guard of the trained convolution{'s' if len(guards) > 1 else ''}: bound "
                       f"{max(guards):.3e} > {model.RANGE_GUARD_LIMIT:.1e}; fit with precision='f32'")
    for layer in [head] + layers:
        layer.write_back(model)
    return history


def fit_head(model, image_units, gt_voxels, *, loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float,
             optimizer: str = "adam", cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit ``model.UNet.pred`` to ground-truth voxels with the rest of the network frozen.

    ``image_units`` [B, L, 2, H, W] with ``gt_voxels`` [B, L, 20, H, W] (f32, on the model's device), or lists of such
    windows; step k works on window k % len(windows).  ``loss`` and ``loss_options`` are those of
    ``losses.calculate_loss``; ``optimizer`` is 'adam' or 'sgd' (plain, no momentum) at learning rate ``lr``.

    The features of a window are computed once and kept while the kept ones fit in ``cache_bytes``; a window beyond the
    budget is recomputed at each of its steps.  Every feature pass starts from the spectral-norm state the model had on
    entry, so a window's features do not depend on whether they were cached.

    Returns the history: per step ``{"loss": float, "loss_dict": {name: float}}``, the values before that step's
    update.  On return the model differs from its state on entry in ``UNet.pred.conv3d.weight`` and ``.bias`` only:
    the spectral-norm u / v and the call counter are restored."""
    return _fit(model, image_units, gt_voxels, allowed=("pred",), train=("pred",), loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


TAIL_GROUPS = ("pred", "conv2", "bn2")


def fit_tail(model, image_units, gt_voxels, *, train: Sequence[str] = TAIL_GROUPS, loss: Sequence[str] = losses.DEFAULT_LOSS,
             steps: int, lr: float, optimizer: str = "adam", cache_bytes: int = DEFAULT_CACHE_BYTES,
             **loss_options) -> List[dict]:
    """Fit the tail of the network -- the last decoder convolution ``UNet.decoders[3].conv2`` with its ``bn2``, and
    ``UNet.pred`` -- to ground-truth voxels with everything in front of it frozen.

    ``train`` names the parameter groups one optimizer steps: 'pred' (the head's weight and bias), 'conv2' (the
    convolution's ``weight_bar``), 'bn2' (the BatchNorm's weight and bias; its statistics stay frozen).  The other
    arguments and the returned history are those of ``fit_head``.

    The two inputs of the convolution (``V2ce3d.forward_tail_inputs``) are cached per window; every step is ``LastConv`` ->
    ``PredHead`` -> the loss.  As in the reference, every forward of the trained convolution advances its spectral-norm
    u / v by one power iteration.  With neither 'conv2' nor 'bn2' in ``train`` the features in front of the head are
    constant and this is ``fit_head``, step for step.

    On return the model differs from its state on entry in the trained tensors and in conv2's ``weight_u`` /
    ``weight_v``, which keep the iterations the fit applied; the other eleven spectral-norm layers and the call counter
    are restored."""
    return _fit(model, image_units, gt_voxels, allowed=TAIL_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


TAIL_NORM_GROUPS = TAIL_GROUPS + ("bn1", "bnd")


def fit_tail_norms(model, image_units, gt_voxels, *, train: Sequence[str] = TAIL_NORM_GROUPS,
                   loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float, optimizer: str = "adam",
                   cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit the whole affine tail of the last decoder block: what ``fit_tail`` trains, and the affine parameters of the
    block's other two BatchNorms -- ``bn1`` behind conv1 and ``downsample.1`` on the shortcut -- whose gradients pass
    through conv2 (``v2ce_conv32_dgrad``).

    ``train`` names the parameter groups one optimizer steps: those of ``fit_tail`` ('pred', 'conv2', 'bn2'), 'bn1' and
    'bnd' (weight and bias each; the statistics stay frozen).  The other arguments and the returned history are those
    of ``fit_tail``.  With neither 'bn1' nor 'bnd' in ``train`` this is ``fit_tail`` with the same arguments, step for
    step.

    The normalised, pre-affine pair in front of the two BatchNorms' affine parts (``V2ce3d.forward_tail_normed``) is
    cached per window; every step is ``TailNorms`` -> ``LastConv`` -> ``PredHead`` -> the loss.

    On return the model differs from its state on entry in the trained tensors and in conv2's ``weight_u`` /
    ``weight_v``, which keep the iterations the fit applied; the other eleven spectral-norm layers and the call counter
    are restored."""
    return _fit(model, image_units, gt_voxels, allowed=TAIL_NORM_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


LAST_BLOCK_GROUPS = TAIL_NORM_GROUPS + ("conv1", "convd")


def fit_last_block(model, image_units, gt_voxels, *, train: Sequence[str] = LAST_BLOCK_GROUPS,
                   loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float, optimizer: str = "adam",
                   cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit the whole last decoder block ``UNet.decoders[3]`` and ``UNet.pred``: what ``fit_tail_norms`` trains, the block's
    spectral-normalised 3x3x3 ``conv1`` and its 1x1x1 shortcut convolution ``downsample.0``, whose weight gradients read
    the block's upsample + concat input without materialising it (``v2ce_convup_wgrad``).

    ``train`` names the parameter groups one optimizer steps: those of ``fit_tail_norms`` ('pred', 'conv2', 'bn2', 'bn1',
    'bnd'), 'conv1' (the convolution's ``weight_bar``) and 'convd' (the shortcut's weight and, where the model has one,
    bias).  The other arguments and the returned history are those of ``fit_tail_norms``.  With neither 'conv1' nor
    'convd' in ``train`` this is ``fit_tail_norms`` with the same arguments, step for step.

    The block's two sources (``V2ce3d.forward_tail_sources``) are cached per window; every step is ``TailConvs`` ->
    ``TailNorms`` -> ``LastConv`` -> ``PredHead`` -> the loss.  As in the reference, every forward of a trained
    convolution advances its spectral-norm u / v by one power iteration.

    On return the model differs from its state on entry in the trained tensors and in the ``weight_u`` / ``weight_v`` of
    the block's conv1 and conv2, which keep the iterations the fit applied; the other ten spectral-norm layers and the
    call counter are restored."""
    return _fit(model, image_units, gt_voxels, allowed=LAST_BLOCK_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


DEC2_CONV_GROUPS = LAST_BLOCK_GROUPS + ("dec2_conv2", "dec2_bn2")


def fit_dec2_conv(model, image_units, gt_voxels, *, train: Sequence[str] = DEC2_CONV_GROUPS,
                  loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float, optimizer: str = "adam",
                  cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit the last decoder block, ``UNet.pred`` and the layer in front of them: what ``fit_last_block`` trains, and the
    second convolution of ``UNet.decoders[2]`` -- the spectral-normalised 3x3x3 ``Conv3d(64, 64)`` that produces the last
    block's source -- with its ``bn2``, whose gradients arrive through the last block's upsample (``v2ce_convup_dgrad``) and
    are formed by ``v2ce_convn_wgrad``.

    ``train`` names the parameter groups one optimizer steps: those of ``fit_last_block``, 'dec2_conv2' (the
    convolution's ``weight_bar``) and 'dec2_bn2' (the BatchNorm's weight and bias; its statistics stay frozen).  The
    other arguments and the returned history are those of ``fit_last_block``.  With neither 'dec2_conv2' nor 'dec2_bn2' in
    ``train`` this is ``fit_last_block`` with the same arguments, step for step.

    The two inputs of the convolution and the last block's skip tensor (``V2ce3d.forward_dec2_inputs``) are cached per
    window; every step is ``Dec2Conv`` -> ``LastBlock`` -> ``PredHead`` -> the loss.  The last block is asked for the
    gradient of its source alone: the skip tensor requires none.  As in the reference, every forward of a trained
    convolution advances its spectral-norm u / v by one power iteration.

    On return the model differs from its state on entry in the trained tensors and in the ``weight_u`` / ``weight_v`` of
    dec2's conv2 and of the last block's conv1 and conv2, which keep the iterations the fit applied; the other nine
    spectral-norm layers and the call counter are restored."""
    return _fit(model, image_units, gt_voxels, allowed=DEC2_CONV_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


DEC2_BLOCK_GROUPS = DEC2_CONV_GROUPS + ("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd")


def fit_dec2_block(model, image_units, gt_voxels, *, train: Sequence[str] = DEC2_BLOCK_GROUPS,
                   loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float, optimizer: str = "adam",
                   cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit the last two decoder blocks and ``UNet.pred``: what ``fit_dec2_conv`` trains, and the first half of
    ``UNet.decoders[2]`` -- its spectral-normalised 3x3x3 ``conv1`` (192 -> 64), its 1x1x1 shortcut convolution
    ``downsample.0`` and the affine parts of ``bn1`` / ``downsample.1`` -- whose weight gradients read the block's upsample +
    concat input without materialising it (``v2ce_convupn_wgrad``).

    ``train`` names the parameter groups one optimizer steps: those of ``fit_dec2_conv``, 'dec2_conv1' (the convolution's
    ``weight_bar``), 'dec2_convd' (the shortcut's weight and, where the model has one, bias), 'dec2_bn1' and 'dec2_bnd'
    (weight and bias each; the statistics stay frozen).  The other arguments and the returned history are those of
    ``fit_dec2_conv``.  With none of the four in ``train`` this is ``fit_dec2_conv`` with the same arguments, step for step.

    The block's two sources and the last block's skip tensor (``V2ce3d.forward_dec2_sources``) are cached per window;
    every step is ``Dec2Block`` -> ``LastBlock`` -> ``PredHead`` -> the loss.  As in the reference, every forward of a
    trained convolution advances its spectral-norm u / v by one power iteration.

    On return the model differs from its state on entry in the trained tensors and in the ``weight_u`` / ``weight_v`` of
    the two convolutions of each of the two blocks, which keep the iterations the fit applied; the other eight
    spectral-norm layers and the call counter are restored."""
    return _fit(model, image_units, gt_voxels, allowed=DEC2_BLOCK_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


DEC1_CONV_GROUPS = DEC2_BLOCK_GROUPS + ("dec1_conv2", "dec1_bn2")


def fit_dec1_conv(model, image_units, gt_voxels, *, train: Sequence[str] = DEC1_CONV_GROUPS,
                  loss: Sequence[str] = losses.DEFAULT_LOSS, steps: int, lr: float, optimizer: str = "adam",
                  cache_bytes: int = DEFAULT_CACHE_BYTES, **loss_options) -> List[dict]:
    """Fit the last two decoder blocks, ``UNet.pred`` and the layer in front of them: what ``fit_dec2_block`` trains, and
    ``UNet.decoders[1].conv2`` -- the spectral-normalised 3x3x3 ``Conv3d(128, 128)`` at a quarter of the resolution whose
    output ``UNet.decoders[2]`` upsamples -- with its ``bn2``, through the input gradient of ``UNet.decoders[2]``'s first
    half (``v2ce_convupn_dgrad``) and the 128-channel gradients of ``v2ce_convc_wgrad`` / ``v2ce_convc_dgrad``.

    ``train`` names the parameter groups one optimizer steps: those of ``fit_dec2_block``, 'dec1_conv2' (the convolution's
    ``weight_bar``) and 'dec1_bn2' (weight and bias; the statistics stay frozen).  The other arguments and the returned
    history are those of ``fit_dec2_block``.  With neither of the two in ``train`` this is ``fit_dec2_block`` with the same
    arguments, step for step.

    The convolution's two inputs and the skip tensors of the two blocks behind it (``V2ce3d.forward_dec1_inputs``) are
    cached per window; every step is ``Dec1Conv`` -> ``Dec2BlockThrough`` (asked for the gradient of ``h1`` alone) ->
    ``LastBlock`` -> ``PredHead`` -> the loss.  As in the reference, every forward of a trained convolution advances its
    spectral-norm u / v by one power iteration.

    On return the model differs from its state on entry in the trained tensors and in the ``weight_u`` / ``weight_v`` of
    ``UNet.decoders[1].conv2`` and of the two convolutions of each of the two blocks behind it, which keep the iterations
    the fit applied; the other seven spectral-norm layers and the call counter are restored."""
    return _fit(model, image_units, gt_voxels, allowed=DEC1_CONV_GROUPS, train=train, loss=loss, steps=steps, lr=lr,
                optimizer=optimizer, cache_bytes=cache_bytes, loss_options=loss_options)


# ---------------------------------------------------------------------------------------------------------------------
# command line

def build_parser():
    p = argparse.ArgumentParser(description="Fit the prediction head of a V2CE checkpoint to a recording")
    p.add_argument("-f", "--image_folder", type=str, help="The folder containing the images")
    p.add_argument("--npy_frames", type=str, help="uint8 [N,H,W] grayscale frames in a .npy file")
    p.add_argument("--synthetic", type=int, default=0, help="generate N synthetic frames instead of reading")
    p.add_argument("--synthetic_weights", type=int, default=None, help="seed of synthetic weights")
    p.add_argument("-m", "--model_path", type=str, default="./weights/v2ce_3d.pt")
    p.add_argument("--precision", type=str, default="f16x2", choices=["f16x2", "f32"])
    p.add_argument("--seq_len", type=int, default=16)
    p.add_argument("--width", type=int, default=346)
    p.add_argument("--height", type=int, default=260)
    p.add_argument("--max_frame_num", type=int, default=1800)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--gt_events", type=str, required=True,
                   help="GT events: .npz with 'event_stream' or a structured .npy (timestamp, x, y, polarity)")
    p.add_argument("--frame_timestamps", type=str, help="int64 us frame times [N] (.npy)")
    p.add_argument("--fps", type=float, default=30, help="without --frame_timestamps: T_i = int(i * 1 / fps * 1e6)")
    p.add_argument("--stage1_losses", "--losses", dest="losses", default=None, nargs="*", metavar="NAME",
                   help="the voxel loss terms (default: pyramid ef ef_splitp compensation; also pt match norml1 norml2)")
    p.add_argument("--ef_type", default="c+cl", choices=("only_c", "cl", "c+cl"))
    p.add_argument("--add_base_loss", action="store_true", help="add the plain MSE to the pyramid loss")
    p.add_argument("--alpha_pyramid", type=float, default=1000)
    p.add_argument("--alpha_ef", type=float, default=0.5)
    p.add_argument("--alpha_efc", type=float, default=5)
    p.add_argument("--alpha_match", type=float, default=0.5)
    p.add_argument("--alpha_compensation", type=float, default=1)
    p.add_argument("--alpha_pt", type=float, default=1)
    p.add_argument("--alpha_norm", type=float, default=1e-5)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--optimizer", default="adam", choices=("adam", "sgd"))
    p.add_argument("--train", default="head", choices=tuple(stage.choice for stage in STAGES),
                   help="head: UNet.pred alone (fit_head); tail: the last decoder convolution, its bn2 and UNet.pred (fit_tail); "
                        "tail_norms: those and the last decoder block's bn1 and downsample.1 (fit_tail_norms); "
                        "last_block: those and the block's conv1 and shortcut convolution, the whole last decoder block "
                        "(fit_last_block); dec2_conv2: those and the second convolution of the decoder in front, UNet.decoders[2].conv2 "
                        "with its bn2 (fit_dec2_conv); dec2_block: those and that decoder's conv1, shortcut convolution, bn1 and downsample.1, "
                        "the whole of UNet.decoders[2] (fit_dec2_block); dec1_conv2: those and the second convolution of the decoder in "
                        "front of that, UNet.decoders[1].conv2 with its bn2 (fit_dec1_conv)")
    p.add_argument("--cache_gb", type=float, default=DEFAULT_CACHE_BYTES / 2 ** 30, help="feature cache budget")
    p.add_argument("-o", "--out", type=str, default="./tuned.pt", help="the tuned state_dict (v2ce.py -m loads it)")
    p.add_argument("--history", type=str, default=None, help="the per-step history as JSON (default: <out>.history.json)")
    p.add_argument("-l", "--log_level", type=str, default="info")
    return p


def recording_windows(frames, gt_events, T, *, seq_len, width, height, device):
    """Frames [N, H, W] uint8, GT events and frame times [N] -> (image-unit windows, GT voxel windows): consecutive
    windows of ``seq_len`` pairs (the last may be shorter), the image units centre-cropped on the width as
    glue.infer_center_image_unit crops them, the GT of each pair voxelised over its own time range as
    stage1_metrics.run_stage1_metric builds it."""
    from . import glue
    from .stage2_metrics import split_by_frames
    from .voxelize import gen_discretized_event_volume_batch
    units = torch.from_numpy(glue.image_pre_processing(np.asarray(frames), height=height))
    fw = units.shape[-1]
    units = units[..., fw // 2 - width // 2: fw // 2 + width // 2].contiguous()
    P, H, W = int(units.shape[0]), int(units.shape[2]), int(units.shape[3])
    gt, counts, dropped = split_by_frames(gt_events, np.asarray(T, dtype=np.int64)[:P + 1])
    logger.info(f"{len(gt)} GT events in {P} pairs; {dropped} outside the frames' time range dropped")
    goff = np.concatenate([[0], np.cumsum(counts)])
    xs, gs = [], []
    for c0 in range(0, P, seq_len):
        c1 = min(P, c0 + seq_len)
        gvol, _ = gen_discretized_event_volume_batch(gt[goff[c0]:goff[c1]], counts[c0:c1], 10, H, W, device=device)
        xs.append(units[c0:c1][None].to(device))
        gs.append(gvol.reshape(1, c1 - c0, 20, H, W).contiguous())
    return xs, gs


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()))
    from . import glue, synth
    from .stage2_metrics import load_events
    from .v2ce import get_trained_mode, read_image_folder
    from .v2ce_3d import V2ce3d
    if str(args.device).startswith("cuda") and torch.device(args.device).index is not None:
        torch.cuda.set_device(torch.device(args.device))
    sources = [args.image_folder, args.npy_frames, args.synthetic or None]
    assert sum(s is not None for s in sources) == 1, "specify exactly one frame source"
    if args.image_folder is not None:
        frames = read_image_folder(args.image_folder, args.max_frame_num)
    elif args.npy_frames is not None:
        frames = np.load(args.npy_frames)[:args.max_frame_num]
    else:
        frames = synth.synthetic_frames(args.synthetic, args.height, args.width)
    if args.synthetic_weights is not None:
        model = V2ce3d(precision=args.precision)
        model.load_state_dict(synth.make_state_dict(args.synthetic_weights))
        model = model.eval().to(args.device)
    else:
        model = get_trained_mode(args.model_path, args.device, args.precision)
    n = len(frames)
    if args.frame_timestamps is not None:
        T = np.load(args.frame_timestamps).astype(np.int64).reshape(-1)
        if T.size < n:
            raise ValueError(f"{args.frame_timestamps}: {T.size} frame times for {n} frames")
        T = T[:n]
    else:
        T = np.array([glue.frame_offset_us(i, args.fps) for i in range(n)], dtype=np.int64)
    xs, gs = recording_windows(frames, load_events(args.gt_events), T, seq_len=args.seq_len, width=args.width,
                               height=args.height, device=args.device)
    names = tuple(args.losses) if args.losses else losses.DEFAULT_LOSS
    opts = {k: getattr(args, k) for k in ("ef_type", "add_base_loss", "alpha_pyramid", "alpha_ef", "alpha_efc",
                                          "alpha_match", "alpha_compensation", "alpha_pt", "alpha_norm")}
    fit = {stage.choice: globals()["fit_" + stage.name] for stage in STAGES}[args.train]
    history = fit(model, xs, gs, loss=names, steps=args.steps, lr=args.lr, optimizer=args.optimizer,
                  cache_bytes=int(args.cache_gb * 2 ** 30), **opts)
    os.makedirs(op.dirname(op.abspath(args.out)), exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, args.out)
    hist_path = args.history or args.out + ".history.json"
    with open(hist_path, "w") as f:
        json.dump({"loss": list(names), "options": opts, "steps": args.steps, "lr": args.lr, "optimizer": args.optimizer,
                   "windows": len(xs), "history": history}, f, indent=1)
    if history:
        logger.info(f"loss {history[0]['loss']:.6g} -> {history[-1]['loss']:.6g} over {len(history)} steps")
    print(args.out)
    print(hist_path)
