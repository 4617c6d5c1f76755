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

from .conv_grads import DGRAD_WANT, TAPS, WGRAD_WANT as WANT, convn_dgrad, convn_wgrad  # noqa: F401
from .decoder_block import Conv2Layer

C = 64                     # channels of dec2.conv2 on either side


class Dec2Conv(Conv2Layer):
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
    C, INDEX = C, 2
    POWER_ITER, BN_FOLD, CHECK_WEIGHT_BAR = "kernel", "sqrt", True
    # the entries, looked up in this module when they are called
    _wgrad = staticmethod(lambda *a, **k: convn_wgrad(*a, **k))
    _dgrad = staticmethod(lambda *a, **k: convn_dgrad(*a, **k))
