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

from .conv_grads import TAPS, UPDGRAD_WANT as DGRAD_WANT, UPWGRAD_WANT as WANT, convup_dgrad, convup_wgrad  # noqa: F401
from .decoder_block import Conv1Layer, DecoderBlock
from .last_conv import LastConv, TailNorms, _planar_pitched  # noqa: F401

C = 32                     # output channels
C0, C1 = 64, 32            # upsampled channels, skip channels
CIN = C0 + C1
_SHAPES = {"weight": (C, CIN, 3, 3, 3), "short": (C, CIN), "short_bias": (C,)}


class TailConvs(Conv1Layer):
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
    C, C0, C1, INDEX = C, C0, C1, 1
    POWER_ITER, SHORTCUT, DGRAD, CHECK_WEIGHT_BAR = "torch", "fused", True, False
    NO_INPUT_GRADS = ("TailConvs provides no gradient with respect to x0 and x1 (the input gradients of conv1 and of the "
                      "shortcut are not implemented): pass tensors that do not require grad")
    # the entries, looked up in this module when they are called
    _wgrad = staticmethod(lambda *a, **k: convup_wgrad(*a, **k))
    _dgrad = staticmethod(lambda *a, **k: convup_dgrad(*a, **k))


class LastBlock(DecoderBlock):
    """The reference's whole last decoder block ``ResidualBlock3D(96, 32, norm='BN', sn=True)`` on
    ``cat(nearest_upsample_2x(x0), x1)`` as one layer: ``TailConvs(input_grads=True) -> TailNorms -> LastConv``, in
    ``.eval()`` (frozen BatchNorm statistics), differentiable in its ten parameter tensors and in both inputs.

        block = LastBlock.from_model(model)
        feat = block(x0, x1)                          # the features ``PredHead`` takes, with a grad_fn
        ... .backward()                               # block.convs / .norms / .conv parameters, x0.grad, x1.grad
        block.write_back(model)

    ``x0.grad`` is the gradient with respect to the block's source as the block reads it, channels-last-16 in ``x0``'s own
    shape with zeros in the padding columns; the relu of the decoder in front (``x0 > 0``) is not applied."""
    CONVS, NORMS, CONV = TailConvs, TailNorms, LastConv
