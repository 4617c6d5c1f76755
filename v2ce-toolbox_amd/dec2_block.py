"""The first half of the third decoder block -- the spectral-normalised 3x3x3 ``conv1`` and the 1x1x1 shortcut convolution
``downsample.0`` of ``UNet.decoders[2]``, both ``Conv3d(192, 64)`` on ``cat(nearest_upsample_2x(dec1 output), skip)``, with
the affine parts of ``bn1`` / ``downsample.1`` -- as trainable layers on the GPU, the whole block as one layer, and the
weight and input gradients through the upsample + concat at any of the decoders' channel counts that they stand on
(include/v2ce_hip_convupngrad.h, csrc/convupnwgrad.hip: the checked entry ``convupn_wgrad``;
include/v2ce_hip_convupndgrad.h, csrc/convupdgrad.hip: ``convupn_dgrad``).

    h1, s2, x1 = model.forward_dec2_sources(x)    # the frozen trunk up to dec2's two sources and dec3's skip tensor
    dec2 = Dec2Block.from_model(model)            # Dec2Convs -> Dec2Norms -> Dec2Conv: ten parameter tensors
    block, head = LastBlock.from_model(model), PredHead.from_model(model)
    pred = head(block(dec2(h1, s2), x1))          # [B, L, 20, H, W], carries a grad_fn
    losses.calculate_loss(pred, gt)[0].backward() # dec2.convs.weight_bar.grad, dec2.convs.short_weight.grad, ...
    for m in (dec2, block, head): m.write_back(model)

With ``Dec2Conv`` (dec2_conv.py) this is the reference's whole ``ResidualBlock3D(192, 64, norm='BN', sn=True)``
(train/scripts/model/submodules.py:249-264) at half the output resolution.  The channel counts of ``convupn_wgrad`` are read
from the tensors; 64 + 32 -> 32 restates ``last_block.convup_wgrad`` byte for byte, and ``convupn_dgrad`` at 64 + 32 -> 32
``last_block.convup_dgrad``.

The gradient with respect to the two sources is ``convupn_dgrad`` at 128 + 64 -> 64, and the layers that return it are
classes of their own: ``Dec2ConvsThrough`` (built with ``input_grads=True``) and ``Dec2BlockThrough``,

    dec2 = Dec2BlockThrough.from_model(model)     # the same ten parameters and state_dict keys as Dec2Block
    h1 = mine(h1)                                 # a layer of the caller's own in front of a source
    ... .backward()                               # h1.grad [B, L, 8, H / 4, ..] and s2.grad [B, L, 4, H / 2, ..] as well

while ``Dec2Convs`` and ``Dec2Block`` keep refusing sources that require grad, as they always have, so ``fit_dec2_block``
trains what it trained.  The package's own layer in front of ``h1`` is ``dec1_conv.Dec1Conv`` (``UNet.decoders[1].conv2``),
and ``finetune.fit_dec1_conv`` trains it through ``Dec2BlockThrough``.  There is no CPU path.
"""
from __future__ import annotations

from .conv_grads import TAPS, UPDGRAD_WANT as DGRAD_WANT, UPWGRAD_WANT as WANT, convupn_dgrad, convupn_wgrad  # noqa: F401
from .dec2_conv import Dec2Conv
from .decoder_block import Conv1Layer, DecoderBlock, NormsLayer

C = 64                     # output channels of dec2.conv1 and of the shortcut
C0, C1 = 128, 64           # upsampled channels, skip channels
CIN = C0 + C1


class Dec2Convs(Conv1Layer):
    """``UNet.decoders[2].conv1`` and ``.downsample[0]`` with the normalising halves of ``bn1`` and ``downsample[1]`` as a
    trainable module, the layer in ``.eval()``: ``TailConvs`` (last_block.py) at 128 + 64 -> 64.  The BatchNorm statistics
    are frozen buffers (their affine parts are ``Dec2Norms``'), conv1's ``weight_bar`` and the shortcut's weight (and bias,
    where the model has one) train.  Like the reference's ``SpectralNorm``, every ``forward`` advances ``weight_u`` /
    ``weight_v`` by one power iteration (no gradient; the model's own kernel ``v2ce_sn_power_iter``, and the sigma it leaves
    is the one the forward's planes are divided by, so the exact-f32 forward has the model's bytes) and divides
    ``weight_bar`` by sigma = u . (W_bar v), through which the gradient does flow.

        z1 = (conv1(X; W_bar / sigma) - mean1) rsqrt(var1 + eps),  zd = (conv_d(X) + bias_d - mean_d) rsqrt(var_d + eps)

    on X = cat(nearest_upsample_2x(x0), x1): what ``V2ce3d.forward_dec2_normed`` returns, with a ``grad_fn``.

    The launches are those ``forward_dec2_inputs`` makes for this block: conv1's and the shortcut's own 1x1x1 launch (in
    ``f16x2`` the model's default path folds the shortcut into conv2's K loop instead).  In ``f16x2`` conv1 is the single
    phase-folded launch on planes of ``W_bar / sigma`` packed at every forward (``v2ce_pack_weights_f16x2_up``): the pair of
    a phase-folded partial launch and a Winograd-T launch on the skip channels, which the model makes for the wider
    decoders, needs the transformed skip planes that ``_prepare`` packs once, and is not made here.  The model packs
    ``W_bar`` once and carries 1 / sigma in the epilogue scale, so in ``f16x2`` the forward is within the split-half
    bound of the model's, not byte-equal.

    ``x0`` and ``x1`` get no gradient from this class: a forward on inputs that require one raises, and so does
    ``input_grads=True``.  ``Dec2ConvsThrough`` is the same layer with that gradient.  ``guard`` (``f16x2``) holds the
    largest range-guard bound of the layer's launches."""
    C, C0, C1, INDEX = C, C0, C1, 2
    POWER_ITER, SHORTCUT, DGRAD, CHECK_WEIGHT_BAR = "kernel", "own", False, True
    NO_INPUT_GRADS = ("Dec2Convs provides no gradient with respect to x0 and x1 (the input gradient of conv1 and of the "
                      "shortcut through the upsample, convupn_dgrad at 128 + 64 -> 64, is Dec2ConvsThrough's, built with "
                      "input_grads=True, and Dec2BlockThrough's): pass tensors that do not require grad")
    # the entry, looked up in this module when it is called
    _wgrad = staticmethod(lambda *a, **k: convupn_wgrad(*a, **k))


class Dec2ConvsThrough(Dec2Convs):
    """``Dec2Convs`` with the gradient with respect to its two sources.  Built with ``input_grads=True`` (``from_model(model,
    input_grads=True)``), a forward takes sources that require grad and the backward returns, next to the parameters'
    gradients, ``d_x0`` (128 channels at the source resolution, a quarter of the network's) and ``d_x1`` (64 channels at
    half): one ``convupn_dgrad`` call on the two weights with the normalisations folded in, only for the sources that
    need it.  Built with ``input_grads=False`` it is ``Dec2Convs``.  The parameters, the buffers and the forward's bytes are
    ``Dec2Convs``': either loads the other's ``state_dict``."""
    DGRAD = True
    NO_INPUT_GRADS = ("this Dec2ConvsThrough was built with input_grads=False and provides no gradient with respect to x0 and "
                      "x1: build it with input_grads=True, or pass tensors that do not require grad")
    # the entry, looked up in this module when it is called
    _dgrad = staticmethod(lambda *a, **k: convupn_dgrad(*a, **k))


class Dec2Norms(NormsLayer):
    """The affine parts of ``UNet.decoders[2]``'s ``bn1`` (behind conv1) and ``downsample.1`` (on the shortcut) as a
    trainable module on the pair ``V2ce3d.forward_dec2_normed`` returns: ``TailNorms`` (last_conv.py) at 64 channels.

        t2, res2 = norms(z1, zd)                      # relu(w1 z1 + b1), wd zd + bd: what Dec2Conv takes

    The statistics stay frozen (the layer in ``.eval()``).  The forward and its per-channel gradient sums are torch
    expressions over the columns ``[..., :lw, :]`` only: the padding columns of ``z1`` / ``zd`` are uninitialised and never
    enter a sum; those of the returned tensors are zeros.  ``t2`` carries ``.absmax``, the range slot a producing launch
    would have left."""
    C, INDEX = C, 2


class Dec2Block(DecoderBlock):
    """The reference's whole third decoder block ``ResidualBlock3D(192, 64, norm='BN', sn=True)`` on
    ``cat(nearest_upsample_2x(x0), x1)`` as one layer: ``Dec2Convs -> Dec2Norms -> Dec2Conv``, in ``.eval()`` (frozen
    BatchNorm statistics), differentiable in its ten parameter tensors.

        dec2 = Dec2Block.from_model(model)
        x0_last = dec2(h1, s2)                        # the source ``LastBlock`` upsamples, with ``.absmax`` and a grad_fn
        ... .backward()                               # dec2.convs / .norms / .conv parameters
        dec2.write_back(model)

    The two sources get no gradient (``Dec2Convs``); ``Dec2BlockThrough`` is the block that gives them one."""
    CONVS, NORMS, CONV = Dec2Convs, Dec2Norms, Dec2Conv


class Dec2BlockThrough(DecoderBlock):
    """``Dec2Block`` differentiable in both sources as well: ``Dec2ConvsThrough`` (input gradients on) ``-> Dec2Norms ->
    Dec2Conv``.  A layer of the caller's own in front of ``h1`` or ``s2`` trains through it:

        dec2 = Dec2BlockThrough.from_model(model)
        x0_last = dec2(mine(h1), s2)                  # sources that require grad are taken
        ... .backward()                               # mine's parameters, through d_x0 = convupn_dgrad(...)['x0']

    The ten parameters and the ``state_dict`` keys are ``Dec2Block``'s, and on sources that do not require grad so is every
    byte of the forward and of the parameters' gradients."""
    CONVS, NORMS, CONV = Dec2ConvsThrough, Dec2Norms, Dec2Conv
