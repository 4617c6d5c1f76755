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

from .conv_grads import DGRAD_WANT, TAPS, WGRAD_WANT as WANT, conv32_dgrad, conv32_wgrad  # noqa: F401
from .decoder_block import Conv2Layer, NormsLayer, _planar_pitched  # noqa: F401

C = 32


class LastConv(Conv2Layer):
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
    C, INDEX = C, 1
    POWER_ITER, BN_FOLD, CHECK_WEIGHT_BAR = "torch", "rsqrt", False
    # the entries, looked up in this module when they are called
    _wgrad = staticmethod(lambda *a, **k: conv32_wgrad(*a, **k))
    _dgrad = staticmethod(lambda *a, **k: conv32_dgrad(*a, **k))


class TailNorms(NormsLayer):
    """The affine parts of the last decoder block's other two BatchNorms -- ``bn1`` behind conv1 and ``downsample.1`` on
    the shortcut -- as a trainable module on the pair ``V2ce3d.forward_tail_normed`` returns:

        z1, zd = model.forward_tail_normed(x)         # normalised, pre-affine, no gradient
        norms = TailNorms.from_model(model)           # bn1_weight, bn1_bias, bnd_weight, bnd_bias [32]
        t, res = norms(z1, zd)                        # relu(w1 z1 + b1), wd zd + bd: what LastConv takes
        head(conv(t, res)) ... .backward()            # the four gradients pass through conv2 (v2ce_conv32_dgrad)

    The statistics stay frozen (the layer in ``.eval()``).  The forward and its per-channel gradient sums are torch
    expressions over the columns ``[..., :lw, :]`` only: the padding columns of ``z1`` / ``zd`` are uninitialised and
    never enter a sum; those of the returned tensors are zeros."""
    C, INDEX = C, 1
