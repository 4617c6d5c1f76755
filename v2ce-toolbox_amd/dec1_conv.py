"""The second convolution of the second decoder block, ``UNet.decoders[1].conv2``, as a trainable layer on the GPU, on the
gradients of a 3x3x3 convolution with any of the UNet's widths (32, 64, 128, 256, 512) on either side
(include/v2ce_hip_convcgrad.h, csrc/convnwgrad.hip, csrc/convndgrad.hip): the checked entries ``convc_wgrad`` and
``convc_dgrad``.

In the reference the layer is the second convolution of ``ResidualBlock3D(384, 128, norm='BN', sn=True)``: a
spectral-normalised 3x3x3 ``Conv3d(128, 128)`` followed by ``bn2``, the shortcut add and ``relu``
(train/scripts/model/submodules.py:249-264), at a quarter of the output resolution.  Its output is ``h1``, the source
``UNet.decoders[2]`` upsamples, and ``Dec2BlockThrough`` (dec2_block.py) returns ``d_h1``: the chain of trainable layers
now reaches back from the prediction head through the last two decoder blocks into the one in front of them,

    t1, res1, s2, x1 = model.forward_dec1_inputs(x)   # the frozen trunk up to dec1.conv2's two inputs and the two skip tensors
    conv = Dec1Conv.from_model(model)                 # weight_bar [128, 128, 3, 3, 3], bn_weight [128], bn_bias [128]
    dec2, block, head = Dec2BlockThrough.from_model(model), LastBlock.from_model(model), PredHead.from_model(model)
    pred = head(block(dec2(conv(t1, res1), s2), x1))  # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward()     # conv.weight_bar.grad, conv.bn_weight.grad, conv.bn_bias.grad, dec2.*, ...
    for m in (conv, dec2, block, head): m.write_back(model)

    Dec1Conv (128 -> 128, 1/4) -> Dec2BlockThrough (128 + 64 -> 64, 1/2) -> LastBlock (64 + 32 -> 32, 1/1) -> PredHead

``dec2`` is asked for the gradient of ``h1`` alone (``s2`` does not require grad).  The channel counts of the two entries
are read from the tensors; at 32 and 64 channels they restate ``dec2_conv.convn_wgrad`` / ``convn_dgrad`` byte for byte.
There is no CPU path.
"""
from __future__ import annotations

from . import hip
from .conv_grads import DGRAD_WANT, TAPS, WGRAD_WANT as WANT, convc_dgrad, convc_wgrad  # noqa: F401
from .decoder_block import Conv2Layer

C = 128                    # channels of dec1.conv2 on either side


class Dec1Conv(Conv2Layer):
    """``UNet.decoders[1].conv2`` + ``bn2`` + shortcut add + relu as a trainable module, the layer in ``.eval()``:
    ``Dec2Conv`` (dec2_conv.py) at 128 channels and a quarter of the resolution, with its policies.  The BatchNorm
    statistics are frozen, its affine parameters and the convolution's ``weight_bar`` train.  Every ``forward`` advances
    ``weight_u`` / ``weight_v`` by one power iteration (no gradient; the model's own kernel, so the exact-f32 forward has
    the model's bytes) and divides ``weight_bar`` by sigma = u . (W_bar v), through which the gradient does flow.  ``t`` and
    ``res`` receive gradients when they require grad (``v2ce_convc_dgrad``: one more launch, none otherwise); like every
    channels-last-16 gradient they have ``t``'s pitch and ``.lw`` and zeros in the padding columns.

    The output is ``h1``, the source ``Dec2BlockThrough`` upsamples, with a ``grad_fn`` and, in ``f16x2``, its range slot
    ``.absmax``.  ``guard`` holds the largest range-guard bound of the layer's launches."""
    C, INDEX = C, 3
    CHANNELS = hip.CONVC_CHANNELS
    POWER_ITER, BN_FOLD, CHECK_WEIGHT_BAR = "kernel", "sqrt", True
    # the entries, looked up in this module when they are called
    _wgrad = staticmethod(lambda *a, **k: convc_wgrad(*a, **k))
    _dgrad = staticmethod(lambda *a, **k: convc_dgrad(*a, **k))
