"""One trainable decoder block ``ResidualBlock3D(c0 + c1, c, norm='BN', sn=True)`` on the GPU, in four roles:

    Conv1Layer    conv1 (spectral-normalised 3x3x3) and the 1x1x1 shortcut ``downsample.0`` on cat(upsample(x0), x1), with
                  the normalising halves of ``bn1`` / ``downsample.1``                        -> (z1, zd)
    NormsLayer    the affine halves of those two BatchNorms, relu on the first              -> (t, res)
    Conv2Layer    conv2 (spectral-normalised 3x3x3) + ``bn2`` + shortcut add + relu         -> the block's output
    DecoderBlock  the three in a row

Each role has one autograd ``Function``; a block of the network is a subclass that sets the channel counts, the block's
index from the end of ``UNet.decoders``, the gradient entries it calls and the policies below.  last_conv.py / last_block.py
hold the subclasses of ``UNet.decoders[-1]`` (32 channels), dec2_conv.py / dec2_block.py those of ``UNet.decoders[-2]`` (64),
dec1_conv.py the conv2 of ``UNet.decoders[-3]`` (128).

The policies are differences between the two blocks that are real: each moves bytes, so each is a named switch and none
is unified here.

    POWER_ITER   'torch': u / v are iterated with torch ``mv`` and the launch weight is packed from W = weight_bar / sigma
                 computed in torch.  'kernel': ``v2ce_sn_power_iter`` iterates them and leaves its sigma in ``_sigma``; the
                 launch weight is packed from ``weight_bar`` with that sigma, as the model packs its own.
    BN_FOLD      (Conv2Layer) 'rsqrt': scale = bn_weight * rsqrt(var + eps).  'sqrt': bn_weight / sqrt(var + eps), as
                 ``V2ce3d._fold_bn``.  They differ in the last bit.
    SHORTCUT     (Conv1Layer, split-half) 'fused': one launch with the shortcut riding on conv1's; the guard is read from
                 z1's range slot.  'own': conv1's and the shortcut's own launch; the guard is read from the whole table.
    DGRAD        (Conv1Layer) does the class have an input-gradient entry ``_dgrad`` (``convup_dgrad`` / ``convupn_dgrad``)?
                 Where it does, a layer built with ``input_grads=True`` returns d_x0 / d_x1 and the forward saves the two
                 weights for it; where it does not, sources that require grad are always refused.
    CHECK_WEIGHT_BAR  refuse a ``weight_bar`` that is not contiguous f32 (it is handed to a kernel as it is).

There is no CPU path.
"""
from __future__ import annotations

import contextlib

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip
from .conv_grads import TAPS, check_sources
from .pred_head import _check_c16


def _planar_pitched(x: torch.Tensor) -> torch.Tensor:
    """Channels-last-16 -> planar [B, T, C, H, pitch] with the padding columns kept (what the exact-f32 launches take as a
    residual: its pitch is the output's)."""
    B, T, G, H, Wp, _ = x.shape
    y = x.permute(0, 1, 2, 5, 3, 4).reshape(B, T, G * 16, H, Wp).contiguous()
    y.lw = getattr(x, "lw", Wp)
    return y


def _decoder(model, index):
    """``model.UNet.decoders[-index]``."""
    if len(model.UNet.decoders) < index:
        raise ValueError("the model has no decoder in front of the last one" if index == 2 else
                         f"the model has fewer than {index} decoders")
    return model.UNet.decoders[-index]


@contextlib.contextmanager
def _own_table(model, slots, batch, dev):
    """The launches inside take their range slots from the model's table: a table of this call's own with ``slots`` rows,
    the model's put back afterwards."""
    P = model._prep
    saved = (P["absmax"], getattr(model, "_slot", 0))
    P["absmax"], model._slot = torch.zeros((slots, batch, 2), dtype=torch.float32, device=dev), 0
    try:
        yield P["absmax"]
    finally:
        P["absmax"], model._slot = saved


class _SpectralConv(nn.Module):
    """What the two convolution roles share: ``weight_bar`` [C, CIN, 3, 3, 3] with ``weight_u`` / ``weight_v``, the power
    iteration, the pack of the launch weight, the model they launch through."""
    C = C0 = C1 = INDEX = 0
    POWER_ITER = "torch"
    CHECK_WEIGHT_BAR = False

    @property
    def CIN(self):
        """conv1 reads the C0 upsampled and the C1 skip channels, conv2 the block's own C."""
        return self.C0 + self.C1 if self.C0 else self.C

    def _init_buffers(self, model, stats):
        self.register_buffer("weight_u", torch.zeros(self.C))
        self.register_buffer("weight_v", torch.zeros(self.CIN * TAPS))
        for n in stats:                                  # frozen BatchNorm statistics
            self.register_buffer(n, (torch.ones if n.endswith("var") else torch.zeros)(self.C))
        self.register_buffer("eps", torch.tensor(1e-5))
        self.register_buffer("guard", torch.zeros(1))   # largest split-half range-guard bound of this layer's launches
        self._model = [model]                            # (a list: the model is not a submodule of this layer)
        self._sigma = self._sn_ws = None

    def _launch_model(self):
        model = self._model[0]
        if model is None:
            name = type(self).__name__
            raise ValueError(f"{name} needs the model whose convolution path it launches: {name}.from_model(model)")
        return model

    def _check_weight_bar(self):
        if self.CHECK_WEIGHT_BAR and (not self.weight_bar.is_contiguous() or self.weight_bar.dtype != torch.float32):
            raise ValueError("weight_bar must be a contiguous float32 tensor")

    def _normalised(self):
        """-> W = weight_bar / sigma as a differentiable tensor, after one power iteration on u / v
        (spectral_norm.py:19-31) by ``POWER_ITER``."""
        w2 = self.weight_bar.view(self.C, -1)
        if self.POWER_ITER == "kernel":
            dev = self.weight_bar.device
            rows, cols = self.C, self.CIN * TAPS
            with torch.no_grad(), torch.cuda.device(dev):
                if self._sigma is None or self._sigma.device != dev:
                    self._sigma = torch.empty(1, dtype=torch.float32, device=dev)
                    self._sn_ws = torch.empty(max(hip.lib().v2ce_sn_workspace_bytes(rows, cols), 16), dtype=torch.uint8, device=dev)
                hip.check(hip.lib().v2ce_sn_power_iter(self.weight_u.data_ptr(), self.weight_v.data_ptr(),
                                                       self.weight_bar.data_ptr(), rows, cols, self._sigma.data_ptr(),
                                                       self._sn_ws.data_ptr(), self._sn_ws.numel(), hip.stream_ptr(dev)),
                          "v2ce_sn_power_iter")
        else:
            with torch.no_grad():
                wd = w2.detach()
                v = torch.mv(wd.t(), self.weight_u)
                self.weight_v.copy_(v / (v.norm() + 1e-12))
                u = torch.mv(wd, self.weight_v)
                self.weight_u.copy_(u / (u.norm() + 1e-12))
        sigma = self.weight_u.dot(w2.mv(self.weight_v))
        return self.weight_bar / sigma

    def _pack(self, model, W, out, split):
        """The launch weight: W (= weight_bar / sigma from torch) or, with the kernel's iteration, weight_bar and its sigma."""
        if self.POWER_ITER == "kernel":
            return model._pack(self.weight_bar.detach().contiguous(), self._sigma, out, split=split)
        return model._pack(W, None, out, split=split)

    def _copy_conv(self, src, dst):
        for n in ("weight_bar", "weight_u", "weight_v"):
            getattr(dst, n).copy_(getattr(src, n).detach())


# ---------------------------------------------------------------------------------------------------------------------
# conv2 + bn2 + shortcut add + relu

class _Conv2Fn(torch.autograd.Function):
    """forward: feat = relu(scale * conv(t, W) + shift + res) as one launch of the model's convolution path; backward: one
    weight-gradient call with the layer's own output as y (the relu's mask), then dW = scale dM, d_scale = <W, dM>,
    d_shift; and, when t or res requires grad, one input-gradient call on the weight with bn2's scale folded in
    (scale[co] W[co], products in torch: one more rounding per term) for d_t and d_res = the masked upstream.

    ``.c16`` / ``.lw``: autograd hands the returned gradients on as plain tensors without the attributes; all the same a
    gradient has the layout, the pitch and the ``.lw`` of the tensor it belongs to, and zeros in its padding columns."""

    @staticmethod
    def forward(ctx, t, res, W, scale, shift, layer):
        model, C = layer._model[0], layer.C
        split = model.precision == "f16x2"
        with torch.no_grad(), torch.cuda.device(t.device):
            if model._prep is None:
                model._prepare()
            Wd = W.detach().contiguous()
            packed = layer._pack(model, Wd, None, split)
            sc, sh = scale.detach().contiguous(), shift.detach().contiguous()
            with _own_table(model, 1, t.shape[0], t.device):
                if split:
                    feat = model._conv(t, None, packed, sc, sh, C, 3, 1, hip.ACT_RELU, residual=res, split=True, track=True)
                    torch.maximum(layer.guard, feat.absmax[:, 1].max().reshape(1), out=layer.guard)
                    layer._slot_out = feat.absmax        # this call's table: the range slot of the layer's output
                    del feat.absmax
                else:
                    y = model._conv(_planar_pitched(t), None, packed, sc, sh, C, 3, 1, hip.ACT_RELU,
                                    residual=_planar_pitched(res), split=False)
                    feat = model.to_c16(y)
                    lw = getattr(t, "lw", t.shape[4])
                    if feat.shape[4] > lw:               # (the exact-f32 launch never writes its padding columns, and
                        feat[:, :, :, :, lw:, :] = 0     # torch.empty hands out whatever an earlier tensor left there)
                    layer._slot_out = None
        ctx.save_for_backward(t, feat, Wd, sc)
        ctx.lw, ctx.layer = getattr(t, "lw", t.shape[4]), layer
        feat.lw, feat.c16 = ctx.lw, True
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        t, feat, W, scale = ctx.saved_tensors
        need_t, need_res, need_w, need_scale, need_shift = ctx.needs_input_grad[:5]
        if not (need_t or need_res or need_w or need_scale or need_shift):
            return (None,) * 6
        layer, C = ctx.layer, ctx.layer.C
        t.lw = feat.lw = ctx.lw                         # (attributes do not survive save_for_backward on every version)
        g = grad_output.contiguous()
        g.lw = ctx.lw
        dW = d_scale = d_shift = d_t = d_res = None
        want = (("weight",) if need_w or need_scale else ()) + (("shift",) if need_shift else ())
        if want:
            r = layer._wgrad(t, feat, g, want=want)
            dM = r.get("weight")
            dW = scale.view(C, 1, 1, 1, 1) * dM if need_w else None
            d_scale = (W * dM).sum(dim=(1, 2, 3, 4)) if need_scale else None
            d_shift = r.get("shift")
        want = (("x",) if need_t else ()) + (("res",) if need_res else ())
        if want:
            r = layer._dgrad((scale.view(C, 1, 1, 1, 1) * W).contiguous(), feat, g, want=want)
            d_t, d_res = r.get("x"), r.get("res")
        return d_t, d_res, dW, d_scale, d_shift, None


class Conv2Layer(_SpectralConv):
    """``conv2`` + ``bn2`` + shortcut add + relu of ``UNet.decoders[-INDEX]`` as a trainable module, the layer in
    ``.eval()``: the BatchNorm statistics are frozen, its affine parameters and the convolution's ``weight_bar`` [C, C, 3, 3,
    3] train.  A subclass sets ``C``, ``INDEX``, the policies, ``_wgrad`` / ``_dgrad``, the two gradient entries, and, where
    those take more than ``hip.CONVN_CHANNELS``, ``CHANNELS``: the channel counts a tensor may have at all (what the
    refusal of a tensor in another layout names)."""
    BN_FOLD = "rsqrt"
    CHANNELS = hip.CONVN_CHANNELS

    def __init__(self, model=None):
        super().__init__()
        C = self.C
        self.weight_bar = nn.Parameter(torch.zeros(C, C, 3, 3, 3))
        self.bn_weight = nn.Parameter(torch.ones(C))
        self.bn_bias = nn.Parameter(torch.zeros(C))
        self._init_buffers(model, ("running_mean", "running_var"))
        self._slot_out = None

    @classmethod
    def from_model(cls, model):
        """A layer holding copies of ``model.UNet.decoders[-INDEX].conv2.module``'s weight_bar / weight_u / weight_v and of
        ``.bn2``'s tensors, on their device; its forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = _decoder(model, cls.INDEX)
        inner, bn = blk.conv2.module, blk.bn2
        if tuple(inner.weight_bar.shape) != (cls.C, cls.C, 3, 3, 3):
            raise ValueError(f"conv2 of UNet.decoders[-{cls.INDEX}] is {tuple(inner.weight_bar.shape)}, not "
                             f"{[cls.C, cls.C, 3, 3, 3]}")
        layer = cls(model).to(inner.weight_bar.device)
        with torch.no_grad():
            layer._copy_conv(inner, layer)
            layer.bn_weight.copy_(bn.weight.detach())
            layer.bn_bias.copy_(bn.bias.detach())
            layer.running_mean.copy_(bn.running_mean)
            layer.running_var.copy_(bn.running_var)
            layer.eps.fill_(BN_EPS)
        return layer

    def effective(self):
        """-> (W, scale, shift) as differentiable tensors, after one power iteration on u / v; scale and shift fold bn2
        by ``BN_FOLD``."""
        W, var = self._normalised(), self.running_var + self.eps
        scale = self.bn_weight / torch.sqrt(var) if self.BN_FOLD == "sqrt" else self.bn_weight * torch.rsqrt(var)
        shift = self.bn_bias - self.running_mean * scale
        return W, scale, shift

    def forward(self, t: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
        """t, res: channels-last-16 [B, L, C / 16, H, pitch, 16] -> the block's output in the same layout with ``.lw``, in
        ``f16x2`` its range slot ``.absmax`` (max |.| per batch element, what the model's launch leaves) and a
        ``grad_fn``."""
        model, C = self._launch_model(), self.C
        dims = _check_c16(t, "t", self.CHANNELS)
        if dims[0] != C:
            raise ValueError(f"t must have {C} channels [b, l, {C // 16}, h0, pitch0, 16], got {tuple(t.shape)}")
        if _check_c16(res, "res", self.CHANNELS) != dims or res.shape != t.shape or res.device != t.device:
            raise ValueError(f"res {tuple(res.shape)} must match t {tuple(t.shape)}")
        self._check_weight_bar()
        W, scale, shift = self.effective()
        feat = _Conv2Fn.apply(t, res, W, scale, shift, self)
        feat.lw, feat.c16 = dims[4], True
        if self._slot_out is not None:
            feat.absmax, self._slot_out = self._slot_out, None
        return feat

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and bn2's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layer."""
        blk = _decoder(model, self.INDEX)
        self._copy_conv(self, blk.conv2.module)
        blk.bn2.weight.copy_(self.bn_weight.detach())
        blk.bn2.bias.copy_(self.bn_bias.detach())
        model._prep = None


# ---------------------------------------------------------------------------------------------------------------------
# conv1 and the shortcut convolution on cat(upsample(x0), x1), normalised

class _Conv1Fn(torch.autograd.Function):
    """forward: z1 = rs1 conv1(X; W) + shift1 and zd = rsd conv_d(X; Wd) + shift_d as the model's own launches on X =
    cat(upsample(x0), x1), on weight buffers of the layer's own -- split-half: one phase-folded launch with the shortcut
    fused in or conv1's and the shortcut's own (``SHORTCUT``), exact f32: the two unfused launches; backward: one
    weight-gradient call on the gradients of (z1, zd), then dW = rs1[co] dM1[co], dWd = rsd[co] dMd[co], d_bias_d = rsd[co]
    sum gd[co] (the normalisations are per output channel and linear, so they commute with the sums over the positions);
    and, when x0 or x1 requires grad (``DGRAD`` and a layer built with ``input_grads=True``), one ``convup_dgrad`` call on
    the weights with the normalisations folded in (rs1[co] W[co] and rsd[co] Wd[co], products in torch: one more rounding
    per term) for d_x0 and d_x1, only those needed.  Nothing is launched when nothing needs a gradient.  ``.c16`` /
    ``.lw``: as for ``_Conv2Fn``."""

    @staticmethod
    def forward(ctx, x0, x1, W, short_w, short_b, layer):
        model, C = layer._model[0], layer.C
        split = model.precision == "f16x2"
        dev = x1.device
        with torch.no_grad(), torch.cuda.device(dev):
            if model._prep is None:
                model._prepare()
            rs1 = (1.0 / torch.sqrt(layer.bn1_var + layer.eps)).float().contiguous()
            rsd = (1.0 / torch.sqrt(layer.bnd_var + layer.eps)).float().contiguous()
            shift1 = (-layer.bn1_mean * rs1).float().contiguous()
            shift_d = (-layer.bnd_mean * rsd if short_b is None else (short_b.detach() - layer.bnd_mean) * rsd).float().contiguous()
            Wd, Sd = W.detach().contiguous(), short_w.detach().contiguous()
            w1, wd = layer._buffers_for(model, split, dev)
            layer._pack(model, Wd, w1, split)
            model._pack(Sd, None, wd, split=split)
            up_to = (int(x1.shape[3]), int(getattr(x1, "lw", x1.shape[4])))
            with _own_table(model, 2, x1.shape[0], dev) as table:
                if split and layer.SHORTCUT == "fused":
                    assert model._fuse_shortcut(_decoder(model, layer.INDEX)), "the block's shortcut rides on conv1's launch"
                    z1, zd = model._conv(x0, x1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=True,
                                         sc=(wd, rsd, shift_d))
                    torch.maximum(layer.guard, z1.absmax[:, 1].max().reshape(1), out=layer.guard)
                    del z1.absmax                       # (a view of this call's table)
                elif split:
                    z1 = model._conv(x0, x1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=True)
                    zd = model._conv(x0, x1, wd, rsd, shift_d, C, 1, 1, hip.ACT_NONE, up_to=up_to, split=True)
                    torch.maximum(layer.guard, table[:, :, 1].max().reshape(1), out=layer.guard)
                    del z1.absmax, zd.absmax            # (views of this call's table)
                else:
                    p0, p1 = _planar_pitched(x0), _planar_pitched(x1)
                    z1 = model.to_c16(model._conv(p0, p1, w1, rs1, shift1, C, 3, 1, hip.ACT_NONE, up_to=up_to, split=False))
                    zd = model.to_c16(model._conv(p0, p1, wd, rsd, shift_d, C, 1, 1, hip.ACT_NONE, up_to=up_to, split=False))
        ctx.save_for_backward(x0, x1, rs1, rsd, *((Wd, Sd) if layer.DGRAD else ()))
        ctx.lw0, ctx.lw, ctx.layer = getattr(x0, "lw", x0.shape[4]), up_to[1], layer
        for z in (z1, zd):
            z.lw, z.c16 = up_to[1], True
        return z1, zd

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, gd):
        x0, x1, rs1, rsd, *weights = ctx.saved_tensors
        need_x0, need_x1, need_w, need_sw, need_sb = ctx.needs_input_grad[:5]
        layer, C, CIN = ctx.layer, ctx.layer.C, ctx.layer.CIN
        x0.lw, x1.lw = ctx.lw0, ctx.lw                  # (attributes do not survive save_for_backward on every version)
        want = (("weight",) if need_w and g1 is not None else ()) + (("short",) if need_sw and gd is not None else ()) + \
            (("short_bias",) if need_sb and gd is not None else ())
        want_x = (("x0",) if need_x0 else ()) + (("x1",) if need_x1 else ())
        if (g1 is None and gd is None) or not (want or want_x):
            return (None,) * 6
        g1, gd = (None if g is None else g.contiguous() for g in (g1, gd))
        for g in (g1, gd):
            if g is not None:
                g.lw = ctx.lw
        r = layer._wgrad(x0, x1, g1, gd, want=want) if want else {}
        dW = rs1.view(C, 1, 1, 1, 1) * r["weight"] if "weight" in r else None
        d_sw = (rsd.view(C, 1) * r["short"]).view(C, CIN, 1, 1, 1) if "short" in r else None
        d_sb = rsd * r["short_bias"] if "short_bias" in r else None
        d_x0 = d_x1 = None
        if want_x:                                      # (the forward refuses inputs that require grad without DGRAD)
            W, short_w = weights
            rx = layer._dgrad((rs1.view(C, 1, 1, 1, 1) * W).contiguous() if g1 is not None else None,
                              (rsd.view(C, 1) * short_w.view(C, CIN)).contiguous() if gd is not None else None, g1, gd,
                              want=want_x, out={"x0": torch.empty_like(x0)} if need_x0 else None)
            d_x0, d_x1 = rx.get("x0"), rx.get("x1")
        return d_x0, d_x1, dW, d_sw, d_sb, None


class Conv1Layer(_SpectralConv):
    """``conv1`` and ``downsample[0]`` of ``UNet.decoders[-INDEX]`` with the normalising halves of ``bn1`` and
    ``downsample[1]`` as a trainable module, the layer in ``.eval()``: the BatchNorm statistics are frozen buffers (their
    affine parts are the block's ``NormsLayer``'s), conv1's ``weight_bar`` [C, C0 + C1, 3, 3, 3] and the shortcut's weight
    (and bias, where the model has one) train.

        z1 = (conv1(X; W_bar / sigma) - mean1) rsqrt(var1 + eps),  zd = (conv_d(X) + bias_d - mean_d) rsqrt(var_d + eps)

    on X = cat(nearest_upsample_2x(x0), x1).  A subclass sets ``C``, ``C0``, ``C1``, ``INDEX``, the policies, ``_wgrad``
    (and ``_dgrad`` with ``DGRAD``), the gradient entries, and ``NO_INPUT_GRADS``, its refusal of sources that require grad."""
    SHORTCUT = "own"
    DGRAD = False
    NO_INPUT_GRADS = ""

    def __init__(self, model=None, bias: bool = True, input_grads: bool = False):
        super().__init__()
        C, CIN = self.C, self.CIN
        if input_grads and not self.DGRAD:
            raise ValueError(self.NO_INPUT_GRADS)
        self.input_grads = bool(input_grads)
        self.weight_bar = nn.Parameter(torch.zeros(C, CIN, 3, 3, 3))
        self.short_weight = nn.Parameter(torch.zeros(C, CIN, 1, 1, 1))
        if bias:
            self.short_bias = nn.Parameter(torch.zeros(C))
        else:
            self.register_parameter("short_bias", None)
        self._init_buffers(model, ("bn1_mean", "bn1_var", "bnd_mean", "bnd_var"))
        self._bufs = {}

    @classmethod
    def from_model(cls, model, input_grads: bool = False):
        """A layer holding copies of ``model.UNet.decoders[-INDEX]``'s ``conv1.module`` (weight_bar / weight_u / weight_v),
        ``downsample[0]`` (weight, bias) and of the statistics of ``bn1`` and ``downsample[1]``, on their device; its
        forward launches through ``model``."""
        from .v2ce_3d import BN_EPS
        blk = _decoder(model, cls.INDEX)
        inner, short = blk.conv1.module, blk.downsample[0]
        C, CIN = cls.C, cls.C0 + cls.C1
        if tuple(inner.weight_bar.shape) != (C, CIN, 3, 3, 3) or tuple(short.weight.shape) != (C, CIN, 1, 1, 1):
            raise ValueError(f"conv1 of UNet.decoders[-{cls.INDEX}] is {tuple(inner.weight_bar.shape)} and its shortcut "
                             f"{tuple(short.weight.shape)}, not {[C, CIN, 3, 3, 3]} and {[C, CIN, 1, 1, 1]}")
        layer = cls(model, bias=short.bias is not None, input_grads=input_grads).to(inner.weight_bar.device)
        with torch.no_grad():
            layer._copy_conv(inner, layer)
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
        C, CIN = self.C, self.CIN
        key = (split, split and model._upfold(), str(dev))
        if key not in self._bufs:
            if split:
                self._bufs[key] = (model._split_buffer(C, CIN, TAPS, dev, up_c0=self.C0 if model._upfold() else 0),
                                   model._split_buffer(C, CIN, 1, dev))
            else:
                self._bufs[key] = (torch.empty(C * CIN * TAPS, dtype=torch.float32, device=dev),
                                   torch.empty(C * CIN, dtype=torch.float32, device=dev))
        return self._bufs[key]

    effective = _SpectralConv._normalised               # -> conv1's weight W_bar / sigma, after one power iteration

    def forward(self, x0: torch.Tensor, x1: torch.Tensor):
        """x0 [B, L, C0 / 16, H0, pitch0, 16], x1 [B, L, C1 / 16, H, pitch, 16] -> (z1, zd), the pair the block's
        ``NormsLayer`` takes, channels-last-16 [B, L, C / 16, H, pitch', 16] with ``.lw`` and a ``grad_fn``."""
        self._launch_model()
        c0, c1, _, _, _, W, _, _ = check_sources(x0, x1)
        if (c0, c1) != (self.C0, self.C1):
            raise ValueError(f"x0 must have {self.C0} channels and x1 {self.C1}, got {tuple(x0.shape)} and {tuple(x1.shape)}")
        if not (self.DGRAD and self.input_grads) and (x0.requires_grad or x1.requires_grad):
            raise ValueError(self.NO_INPUT_GRADS)
        self._check_weight_bar()
        z1, zd = _Conv1Fn.apply(x0, x1, self.effective(), self.short_weight, self.short_bias, self)
        for z in (z1, zd):
            z.lw, z.c16 = W, True
        return z1, zd

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy weight_bar, u, v and the shortcut's weight and bias into ``model`` and drop its derived constants: the next
        inference call runs the tuned layers."""
        blk = _decoder(model, self.INDEX)
        short = blk.downsample[0]
        self._copy_conv(self, blk.conv1.module)
        short.weight.copy_(self.short_weight.detach())
        if self.short_bias is not None and short.bias is not None:
            short.bias.copy_(self.short_bias.detach())
        model._prep = None


# ---------------------------------------------------------------------------------------------------------------------
# the affine halves of bn1 and downsample.1, and the whole block

class NormsLayer(nn.Module):
    """The affine parts of ``bn1`` (behind conv1) and ``downsample.1`` (on the shortcut) of ``UNet.decoders[-INDEX]`` as a
    trainable module on the pair the block's ``Conv1Layer`` returns: t = relu(w1 z1 + b1), res = wd zd + bd, what its
    ``Conv2Layer`` takes (the subclasses say more).  A subclass sets ``C`` and ``INDEX``."""
    C = INDEX = 0

    def __init__(self):
        super().__init__()
        for n in ("bn1", "bnd"):
            setattr(self, n + "_weight", nn.Parameter(torch.ones(self.C)))
            setattr(self, n + "_bias", nn.Parameter(torch.zeros(self.C)))

    @classmethod
    def _norms(cls, model):
        blk = _decoder(model, cls.INDEX)
        return blk.bn1, blk.downsample[1]

    def _copy(self, model, to_model):
        for n, bn in zip(("bn1", "bnd"), self._norms(model)):
            for a in ("weight", "bias"):
                mine, theirs = getattr(self, f"{n}_{a}"), getattr(bn, a)
                (theirs if to_model else mine).copy_((mine if to_model else theirs).detach())

    @classmethod
    def from_model(cls, model):
        """A module holding copies of the affine parameters of ``model.UNet.decoders[-INDEX]``'s ``bn1`` and
        ``downsample[1]``, on their device."""
        bn1, bnd = cls._norms(model)
        if tuple(bn1.weight.shape) != (cls.C,) or tuple(bnd.weight.shape) != (cls.C,):
            raise ValueError(f"UNet.decoders[-{cls.INDEX}] has {tuple(bn1.weight.shape)} channels, not {[cls.C]}")
        layer = cls().to(bn1.weight.device)
        with torch.no_grad():
            layer._copy(model, False)
        return layer

    def forward(self, z1: torch.Tensor, zd: torch.Tensor):
        """z1, zd: channels-last-16 [B, L, C / 16, H, pitch, 16] -> (t, res) in the same layout with ``.lw``, zeros in the
        padding columns and a ``grad_fn``."""
        C = self.C
        dims = _check_c16(z1, "z1", (C,))
        if _check_c16(zd, "zd", (C,)) != dims or zd.shape != z1.shape or zd.device != z1.device:
            raise ValueError(f"zd {tuple(zd.shape)} must match z1 {tuple(z1.shape)}")
        lw, pitch = dims[4], dims[5]
        per = lambda p: p.view(C // 16, 1, 1, 16)            # channel g * 16 + j of [B, L, g, H, column, j]
        t = torch.relu(per(self.bn1_weight) * z1[..., :lw, :] + per(self.bn1_bias))
        res = per(self.bnd_weight) * zd[..., :lw, :] + per(self.bnd_bias)
        t, res = (nn.functional.pad(a, (0, 0, 0, pitch - lw)).contiguous() for a in (t, res))
        for a in (t, res):
            a.lw, a.c16 = lw, True
        # the range slot of the split-half path: [max |t|, no range-guard value] per batch element, what a producing launch
        # would have left (the padding columns are zeros), so conv2 scales t as it does behind the model's own launch
        amax = t.detach().abs().amax(dim=(1, 2, 3, 4, 5))
        t.absmax = torch.stack([amax, torch.zeros_like(amax)], dim=1).contiguous()
        return t, res

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy the four vectors into ``model`` and drop its derived constants: the next inference call runs the tuned
        BatchNorms."""
        self._copy(model, True)
        model._prep = None


class DecoderBlock(nn.Module):
    """A whole decoder block as one layer, ``CONVS -> NORMS -> CONV`` (the three roles' classes), in ``.eval()`` (frozen
    BatchNorm statistics), differentiable in its ten parameter tensors and, where ``CONVS.DGRAD``, in both inputs."""
    CONVS = NORMS = CONV = None

    def __init__(self, convs, norms, conv):
        super().__init__()
        self.convs, self.norms, self.conv = convs, norms, conv

    @classmethod
    def from_model(cls, model):
        return cls(cls.CONVS.from_model(model, input_grads=cls.CONVS.DGRAD), cls.NORMS.from_model(model),
                   cls.CONV.from_model(model))

    def forward(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """x0 [B, L, C0 / 16, H0, pitch0, 16], x1 [B, L, C1 / 16, H, pitch, 16] -> the block's output [B, L, C / 16, H,
        pitch', 16] with ``.lw``, ``.absmax`` (``f16x2``) and a ``grad_fn``."""
        return self.conv(*self.norms(*self.convs(x0, x1)))

    @torch.no_grad()
    def write_back(self, model) -> None:
        """Copy the three layers' tensors into ``model``: the next inference call runs the tuned block."""
        for m in (self.convs, self.norms, self.conv):
            m.write_back(model)
