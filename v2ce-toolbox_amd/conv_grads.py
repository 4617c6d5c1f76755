"""The checked Python entries of the convolution gradient kernels the trainable decoder layers stand on
(include/v2ce_hip_convgrad.h, v2ce_hip_convdgrad.h, v2ce_hip_convupgrad.h, v2ce_hip_convupdgrad.h, v2ce_hip_convngrad.h,
v2ce_hip_convcgrad.h, v2ce_hip_convupngrad.h, v2ce_hip_convupndgrad.h; csrc/convnwgrad.hip, convndgrad.hip, convupnwgrad.hip, convupdgrad.hip):

    convn_wgrad / convn_dgrad    a stride-1 3x3x3 convolution cin -> cout seen through the relu behind it
    convc_wgrad / convc_dgrad    the same two with cin and cout each any of 32, 64, 128, 256, 512 (v2ce_convc_wgrad,
                                 v2ce_convc_dgrad); convn_* stop at 64
    convupn_wgrad                the 3x3x3 and the 1x1x1 convolution c0 + c1 -> cout on cat(nearest_upsample_2x(x0), x1)
    convupn_dgrad                the input gradients of that pair, back through the concat and the upsample
    conv32_wgrad / conv32_dgrad / convup_wgrad / convup_dgrad
                                 the same four with the channel counts fixed at 32 -> 32 and 64 + 32 -> 32, through C
                                 entries of their own (v2ce_conv32_wgrad, v2ce_conv32_dgrad, v2ce_convup_wgrad,
                                 v2ce_convup_dgrad)

Every entry validates its tensors (``pred_head._check_c16``: channels-last-16 f32 on the device, ``.lw`` inside the pitch,
16-byte aligned), ``want`` / ``out`` / ``max_workgroups``, refuses an output that overlaps an input, queries the workspace
and makes one call without host synchronisation.  last_conv.py, last_block.py, dec2_conv.py and dec2_block.py export them
under the names their layers and tests use.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import hip
from .pred_head import _check_c16, _check_f32, _no_overlap

TAPS = 27
WGRAD_WANT = ("weight", "shift")
DGRAD_WANT = ("x", "res")
UPWGRAD_WANT = ("weight", "short", "short_bias")
UPDGRAD_WANT = ("x0", "x1")
UP_C0, UP_C1, UP_COUT = 64, 32, 32         # the one channel triple of convup_wgrad and convup_dgrad


class _Entry(NamedTuple):
    """A C entry: ``symbol`` and ``symbol + '_workspace_bytes'``, the channel counts its tensors may have (one tuple per
    role) and whether it takes them as arguments."""
    symbol: str
    channels: tuple
    pass_channels: bool


_CONVN_WGRAD = _Entry("v2ce_convn_wgrad", (hip.CONVN_CHANNELS, hip.CONVN_CHANNELS), True)
_CONV32_WGRAD = _Entry("v2ce_conv32_wgrad", ((32,), (32,)), False)
_CONVN_DGRAD = _Entry("v2ce_convn_dgrad", (hip.CONVN_CHANNELS, hip.CONVN_CHANNELS), True)
_CONV32_DGRAD = _Entry("v2ce_conv32_dgrad", ((32,), (32,)), False)
_CONVC_WGRAD = _Entry("v2ce_convc_wgrad", (hip.CONVC_CHANNELS, hip.CONVC_CHANNELS), True)
_CONVC_DGRAD = _Entry("v2ce_convc_dgrad", (hip.CONVC_CHANNELS, hip.CONVC_CHANNELS), True)
_CONVUPN_WGRAD = _Entry("v2ce_convupn_wgrad", (hip.CONVUPN_C0, hip.CONVUPN_C1, hip.CONVUPN_COUT), True)
_CONVUP_WGRAD = _Entry("v2ce_convup_wgrad", ((UP_C0,), (UP_C1,), (UP_COUT,)), False)
_CONVUP_DGRAD = _Entry("v2ce_convup_dgrad", ((UP_C0,), (UP_C1,), (UP_COUT,)), False)
_CONVUPN_DGRAD = _Entry("v2ce_convupn_dgrad", (hip.CONVUPN_C0, hip.CONVUPN_C1, hip.CONVUPN_COUT), True)


def check_sources(x0, x1, c0s=hip.CONVUPN_C0, c1s=hip.CONVUPN_C1):
    """x0 at the source resolution against x1: the same b and l, h0 = (h + 1) // 2, lw0 = (lw + 1) // 2 and a nearest
    upsample that reads its source at (h >> 1, w >> 1) -> (c0, c1, B, L, H, W, pitch, pitch0)."""
    c1, B, L, H, W, pitch = _check_c16(x1, "x1", c1s)
    c0, B0, L0, H0, W0, pitch0 = _check_c16(x0, "x0", c0s)
    if x0.device != x1.device:
        raise ValueError(f"x0 lives on {x0.device}, x1 on {x1.device}")
    if (B0, L0) != (B, L) or H0 != (H + 1) // 2 or W0 != (W + 1) // 2:
        raise ValueError(f"x0 {tuple(x0.shape)} (lw {W0}) must match x1 {tuple(x1.shape)} (lw {W}): the same b and l, "
                         f"h0 = (h + 1) // 2 = {(H + 1) // 2} and lw = {(W + 1) // 2}")
    _check_half(H, W)
    return c0, c1, B, L, H, W, pitch, pitch0


def _check_half(H, W):
    from .v2ce_3d import _nearest_is_half
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    if not (_nearest_is_half(H0, H) and _nearest_is_half(W0, W)):
        raise ValueError(f"the nearest upsample {(H0, W0)} -> {(H, W)} does not read its source at (h >> 1, w >> 1)")


def _check_same(t, name, dims, ref, ref_name, pos, planes=True):
    """t, with ``dims`` = its (B, L, H, W, pitch), against the reference tensor: the device, ``pos`` and, where
    ``planes``, the shape."""
    if t.device != ref.device:
        raise ValueError(f"{name} lives on {t.device}, {ref_name} on {ref.device}")
    if tuple(dims) != tuple(pos) or (planes and tuple(t.shape) != tuple(ref.shape)):
        raise ValueError(f"{name} {tuple(t.shape)} (lw {dims[3]}) must match {ref_name} {tuple(ref.shape)} (lw {pos[3]})"
                         + ("" if planes else " but for the planes"))


def _arguments(want, allowed, max_workgroups):
    want = tuple(want)
    if not want or any(n not in allowed for n in want) or len(set(want)) != len(want):
        raise ValueError(f"want must be a non-empty subset of {allowed}, got {want}")
    if int(max_workgroups) < 0:
        raise ValueError(f"max_workgroups must be >= 0, got {max_workgroups}")
    return want, int(max_workgroups)


def _outputs(out, want, dev, ins, check):
    """The caller's ``out`` checked: wanted names only, f32 on ``dev``, ``check(name, tensor)``, no overlap."""
    out = dict(out or {})
    if any(n not in want for n in out):
        raise ValueError(f"out holds {sorted(out)}, want is {want}")
    for n, t in out.items():
        _check_f32(t, f"out['{n}']", dev)
        check(n, t)
    _no_overlap([(f"out['{n}']", t) for n, t in out.items()], ins)
    return out


def _elements(shapes):
    def check(n, t):
        if t.numel() != torch.Size(shapes[n]).numel():
            raise ValueError(f"out['{n}'] has {t.numel()} elements")
    return check


def _launch(entry, chans, pos, detail, pointers, names, want, out, shapes, cap, dev):
    """Query the workspace, allocate it and the wanted outputs that ``out`` does not hold, make the call: the input
    ``pointers``, the channel counts where the entry takes them, ``pos``, the outputs in the order ``names``, workspace,
    cap and stream.  -> {name: tensor}."""
    lib = hip.lib()
    dims = (tuple(chans) if entry.pass_channels else ()) + tuple(pos)
    nb = getattr(lib, entry.symbol + "_workspace_bytes")(*dims, cap)
    if nb == 0:
        raise hip.V2ceHipError(f"{entry.symbol}: unsupported shape {tuple(pos[:4])} ({detail})")
    with torch.cuda.device(dev):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        res = {n: out[n] if n in out else torch.empty(shapes[n], dtype=torch.float32, device=dev) for n in want}
        hip.check(getattr(lib, entry.symbol)(*pointers, *dims, *(hip.ptr(res.get(n)) for n in names), ws.data_ptr(), nb,
                                             cap, hip.stream_ptr(dev)), entry.symbol)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# a 3x3x3 convolution cin -> cout seen through the relu behind it

def _wgrad(entry, x, y, upstream, want, out, max_workgroups):
    want, cap = _arguments(want, WGRAD_WANT, max_workgroups)
    cin, *pos = _check_c16(x, "x", entry.channels[0])
    cout, *upos = _check_c16(upstream, "upstream", entry.channels[1])
    ins = [("upstream", upstream)]
    if y is not None:
        _check_same(y, "y", _check_c16(y, "y", entry.channels[1])[1:], upstream, "upstream", upos)
        ins.append(("y", y))
    _check_same(upstream, "upstream", upos, x, "x", pos, planes=False)
    ins.append(("x", x))
    shapes = {"weight": (cout, cin, 3, 3, 3), "shift": (cout,)}
    out = _outputs(out, want, x.device, ins, _elements(shapes))
    detail = f"pitch {pos[4]}" + (f", {cin} -> {cout}" if entry.pass_channels else "")
    return _launch(entry, (cin, cout), pos, detail, (x.data_ptr(), hip.ptr(y), upstream.data_ptr()), WGRAD_WANT, want, out,
                   shapes, cap, x.device)


def _dgrad(entry, weight, y, upstream, want, out, max_workgroups):
    want, cap = _arguments(want, DGRAD_WANT, max_workgroups)
    cout, *pos = _check_c16(upstream, "upstream", entry.channels[1])
    dev = upstream.device
    ins = [("upstream", upstream)]
    if y is not None:
        _check_same(y, "y", _check_c16(y, "y", entry.channels[1])[1:], upstream, "upstream", pos)
        ins.append(("y", y))
    _check_f32(weight, "weight", dev)
    cins = entry.channels[0]
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or int(weight.shape[0]) != cout or int(weight.shape[1]) not in cins:
        raise ValueError(f"weight must be [{cout}, {' or '.join(str(c) for c in cins)}, 3, 3, 3] (upstream has {cout} "
                         f"channels), got {tuple(weight.shape)}")
    cin = int(weight.shape[1])
    ins.append(("weight", weight))
    B, L, H, W, pitch = pos
    shapes = {"x": (B, L, cin // 16, H, pitch, 16), "res": tuple(upstream.shape)}

    def check(n, t):
        if tuple(t.shape) != shapes[n]:
            raise ValueError(f"out['{n}'] {tuple(t.shape)} must be {shapes[n]}" if entry.pass_channels else
                             f"out['{n}'] {tuple(t.shape)} must match upstream {tuple(upstream.shape)}")
        if t.data_ptr() % 16:
            raise ValueError(f"out['{n}'] must be 16-byte aligned")
    out = _outputs(out, want, dev, ins, check)
    detail = f"pitch {pitch}" + (f", {cin} -> {cout}" if entry.pass_channels else "")
    res = _launch(entry, (cin, cout), pos, detail, (weight.data_ptr(), hip.ptr(y), upstream.data_ptr()), DGRAD_WANT, want,
                  out, shapes, cap, dev)
    for t in res.values():
        t.lw, t.c16 = W, True
    return res


def convn_wgrad(x: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = WGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu behind it.
    ``x`` (the convolution's input, cin channels), ``y`` (the relu's output, or None: no mask) and ``upstream`` (the
    gradient with respect to ``y``; both cout channels) are channels-last-16 f32 with the same B, L, H, pitch and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'shift'): 'weight' [cout, cin, 3, 3, 3] = sum over
    the positions of m[co] x[ci] shifted by the tap, 'shift' [cout] = sum of m[co], with m = upstream where y > 0 else 0.
    ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the shares of the
    tile walk at max(n / pairs, 1), pairs = (cout / 32) (cin / 32) (the result then depends on n only through the order
    of the f64 sums).  One call, no host synchronisation."""
    return _wgrad(_CONVN_WGRAD, x, y, upstream, want, out, max_workgroups)


def conv32_wgrad(x: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                 want: Sequence[str] = WGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """``convn_wgrad`` at 32 -> 32 through ``v2ce_conv32_wgrad``: every tensor is ``[B, L, 2, H, pitch, 16]``, 'weight'
    [32, 32, 3, 3, 3] and 'shift' [32]; anything else is refused."""
    return _wgrad(_CONV32_WGRAD, x, y, upstream, want, out, max_workgroups)


def convn_dgrad(weight: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = DGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The input gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu behind it.
    ``weight`` is the convolution's own contiguous ``[cout, cin, 3, 3, 3]`` f32 weight; ``y`` (the relu's output, or None:
    no mask) and ``upstream`` (the gradient with respect to ``y``) are channels-last-16 f32 with cout channels, the same
    shape and ``.lw``.  -> {name: tensor} for the names in ``want`` (a subset of 'x', 'res'): 'x' (cin channels) = the
    transposed convolution of m with the weight, 'res' (cout channels) = m, with m = upstream where y > 0 else 0; both
    carry upstream's pitch and ``.lw`` and zeros in the padding columns ``lw .. pitch - 1``.  ``out``: {name: tensor} to
    write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the grid (the bytes do not depend on n).  One
    call, no host synchronisation."""
    return _dgrad(_CONVN_DGRAD, weight, y, upstream, want, out, max_workgroups)


def conv32_dgrad(weight: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                 want: Sequence[str] = DGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """``convn_dgrad`` at 32 -> 32 through ``v2ce_conv32_dgrad``: ``weight`` is ``[32, 32, 3, 3, 3]``, every other tensor
    ``[B, L, 2, H, pitch, 16]``; anything else is refused."""
    return _dgrad(_CONV32_DGRAD, weight, y, upstream, want, out, max_workgroups)


def convc_wgrad(x: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = WGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """``convn_wgrad`` with cin and cout each one of ``hip.CONVC_CHANNELS`` (32, 64, 128, 256, 512), through
    ``v2ce_convc_wgrad``: the weight gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu
    behind it.  ``x`` (the convolution's input, cin channels), ``y`` (the relu's output, or None: no mask) and ``upstream``
    (the gradient with respect to ``y``; both cout channels) are channels-last-16 f32 with the same B, L, H, pitch and
    ``.lw``.  -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'shift'): 'weight' [cout, cin, 3, 3, 3] =
    sum over the positions of m[co] x[ci] shifted by the tap, 'shift' [cout] = sum of m[co], with m = upstream where y > 0
    else 0.  ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the shares of
    the tile walk at max(n / pairs, 1), pairs = (cout / 32) (cin / 32) <= 256 (the result then depends on n only through
    the order of the f64 sums).  At cin, cout in (32, 64) the bytes are ``convn_wgrad``'s.  One call, no host
    synchronisation."""
    return _wgrad(_CONVC_WGRAD, x, y, upstream, want, out, max_workgroups)


def convc_dgrad(weight: torch.Tensor, y: Optional[torch.Tensor], upstream: torch.Tensor, *,
                want: Sequence[str] = DGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """``convn_dgrad`` with cin and cout each one of ``hip.CONVC_CHANNELS`` (32, 64, 128, 256, 512), through
    ``v2ce_convc_dgrad``: the input gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout seen through the relu
    behind it.  ``weight`` is the convolution's own contiguous ``[cout, cin, 3, 3, 3]`` f32 weight; ``y`` (the relu's
    output, or None: no mask) and ``upstream`` (the gradient with respect to ``y``) are channels-last-16 f32 with cout
    channels, the same shape and ``.lw``.  -> {name: tensor} for the names in ``want`` (a subset of 'x', 'res'): 'x' (cin
    channels) = the transposed convolution of m with the weight, 'res' (cout channels) = m, with m = upstream where y > 0
    else 0; both carry upstream's pitch and ``.lw`` and zeros in the padding columns ``lw .. pitch - 1``.  ``out``: {name:
    tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the grid (the bytes do not depend on
    n).  At cin, cout in (32, 64) the bytes are ``convn_dgrad``'s.  One call, no host synchronisation."""
    return _dgrad(_CONVC_DGRAD, weight, y, upstream, want, out, max_workgroups)


# ---------------------------------------------------------------------------------------------------------------------
# the 3x3x3 and the 1x1x1 convolution c0 + c1 -> cout on the virtual tensor X = cat(nearest_upsample_2x(x0), x1)

def _upwgrad(entry, x0, x1, g1, gd, want, out, max_workgroups):
    want, cap = _arguments(want, UPWGRAD_WANT, max_workgroups)
    if "weight" in want and g1 is None:
        raise ValueError("want 'weight' needs g1")
    if ("short" in want or "short_bias" in want) and gd is None:
        raise ValueError("want 'short' and 'short_bias' need gd")
    c0, c1, *pos, pitch0 = check_sources(x0, x1, entry.channels[0], entry.channels[1])
    ins, cout = [("x0", x0), ("x1", x1)], None
    for n, t in (("g1", g1), ("gd", gd)):
        if t is None:
            continue
        co, *dims = _check_c16(t, n, entry.channels[2])
        _check_same(t, n, dims, x1, "x1", pos, planes=False)
        if cout is not None and co != cout:
            raise ValueError(f"gd {tuple(t.shape)} must match g1 {tuple(g1.shape)}")
        cout = co
        ins.append((n, t))
    cin = c0 + c1
    shapes = {"weight": (cout, cin, 3, 3, 3), "short": (cout, cin), "short_bias": (cout,)}
    out = _outputs(out, want, x1.device, ins, _elements(shapes))
    detail = f"pitch {pos[4]}, pitch0 {pitch0}" + (f", {c0} + {c1} -> {cout}" if entry.pass_channels else "")
    return _launch(entry, (c0, c1, cout), (*pos, pitch0), detail,
                   (x0.data_ptr(), x1.data_ptr(), hip.ptr(g1) if "weight" in want else None,
                    hip.ptr(gd) if ("short" in want or "short_bias" in want) else None), UPWGRAD_WANT, want, out, shapes, cap,
                   x1.device)


def convupn_wgrad(x0: torch.Tensor, x1: torch.Tensor, g1: Optional[torch.Tensor], gd: Optional[torch.Tensor], *,
                  want: Sequence[str] = UPWGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """The weight gradients of the 3x3x3 and the 1x1x1 convolution c0 + c1 -> cout on the virtual tensor
    ``X = cat(nearest_upsample_2x(x0), x1)``.  ``x0`` is channels-last-16 ``[B, L, c0 / 16, H0, pitch0, 16]`` f32 (c0 = 64
    or 128) with ``H0 = (H + 1) // 2`` and ``.lw = (W + 1) // 2``; ``x1`` (the skip tensor, c1 = 32 or 64 channels) is
    ``[B, L, c1 / 16, H, pitch, 16]``; ``g1`` (the gradient with respect to the 3x3x3 convolution's output) and ``gd`` (the
    gradient with respect to the 1x1x1 convolution's output) are ``[B, L, cout / 16, H, pitch, 16]`` (cout = 32 or 64) with
    ``x1``'s B, L, H, pitch and ``.lw``.
    -> {name: tensor} for the names in ``want`` (a subset of 'weight', 'short', 'short_bias'): 'weight'
    [cout, c0 + c1, 3, 3, 3] = sum over the positions of g1[co] X[ci] shifted by the tap (zero padding at the upsampled
    resolution), 'short' [cout, c0 + c1] = sum of gd[co] X[ci], 'short_bias' [cout] = sum of gd[co].  ``g1`` may be None
    without 'weight', ``gd`` without 'short' and 'short_bias'.  ``out``: {name: tensor} to write into.  ``max_workgroups``:
    0 = the kernel's choice, n > 0 caps the shares of the tile walk at max(n / pairs, 1), pairs = (cout / 32)
    ((c0 + c1) / 32) (the result then depends on n only through the order of the f64 sums).  One call, no host
    synchronisation."""
    return _upwgrad(_CONVUPN_WGRAD, x0, x1, g1, gd, want, out, max_workgroups)


def convup_wgrad(x0: torch.Tensor, x1: torch.Tensor, g1: Optional[torch.Tensor], gd: Optional[torch.Tensor], *,
                 want: Sequence[str] = UPWGRAD_WANT, out: Optional[dict] = None, max_workgroups: int = 0) -> dict:
    """``convupn_wgrad`` at 64 + 32 -> 32 through ``v2ce_convup_wgrad``: ``x0`` is ``[B, L, 4, H0, pitch0, 16]``, ``x1``,
    ``g1`` and ``gd`` are ``[B, L, 2, H, pitch, 16]``, 'weight' [32, 96, 3, 3, 3], 'short' [32, 96] and 'short_bias' [32];
    anything else is refused."""
    return _upwgrad(_CONVUP_WGRAD, x0, x1, g1, gd, want, out, max_workgroups)


def _resolve_c0(entry, cin, given, c0):
    """How the cin input channels of a weight split into c0 + c1: from out['x0'] (``given``) where it is there, else from
    ``c0``, else from cin alone.  cin alone does not say it where cin is itself one of the entry's c0: 128 input channels
    are 64 + 64, or the 128 channels of an x0 with no skip tensor beside it, which no entry takes -- a caller who means the
    second must hear so and not get the first's gradients.  -> c0, or None where cin is no sum the entry takes."""
    pairs = [(a, b) for a in entry.channels[0] for b in entry.channels[1] if a + b == cin]
    if not pairs:
        return None
    if c0 is None and given is not None and given.dim() == 6:
        c0 = 16 * int(given.shape[2])
    if c0 is None:
        if cin in entry.channels[0]:
            raise ValueError(f"a weight with {cin} input channels reads as {pairs[0][0]} + {pairs[0][1]} or as {cin} + 0 (which "
                             f"is refused): say which with c0={pairs[0][0]} or out['x0']")
        return pairs[0][0]
    if (int(c0), cin - int(c0)) not in pairs:
        raise ValueError(f"c0 = {c0} does not split {cin} input channels into c0 in {tuple(entry.channels[0])} and c1 in "
                         f"{tuple(entry.channels[1])}")
    return int(c0)


def _updgrad(entry, weight, short_weight, g1, gd, want, out, max_workgroups, c0=None):
    from .v2ce_3d import V2ce3d
    want, cap = _arguments(want, UPDGRAD_WANT, max_workgroups)
    if g1 is None and gd is None:
        raise ValueError("g1 and gd are both None")
    if g1 is not None and weight is None:
        raise ValueError("g1 needs weight")
    if gd is not None and short_weight is None:
        raise ValueError("gd needs short_weight")
    given = (out or {}).get("x0")
    first = weight if g1 is not None else short_weight
    cin = int(first.shape[1]) if first.dim() >= 2 else 0
    c0 = _resolve_c0(entry, cin, given, c0)          # an ambiguous call is refused before anything else is looked at
    lead, lead_name = (g1, "g1") if g1 is not None else (gd, "gd")
    cout, B, L, H, W, pitch = _check_c16(lead, lead_name, entry.channels[2])
    dev = lead.device
    ins = [(lead_name, lead)]
    if g1 is not None and gd is not None:
        _check_same(gd, "gd", _check_c16(gd, "gd", entry.channels[2])[1:], g1, "g1", (B, L, H, W, pitch))
        ins.append(("gd", gd))
    # the input channels a weight may have: those the call resolved to, or (where it did not) every sum the entry takes
    cins = (cin,) if c0 is not None else sorted({a + b for a in entry.channels[0] for b in entry.channels[1]})
    for n, t, tails, used in (("weight", weight, ((3, 3, 3),), g1 is not None),
                              ("short_weight", short_weight, ((), (1, 1, 1)), gd is not None)):
        if not used:
            continue
        _check_f32(t, n, dev)
        ok = [(cout, ci) + tail for tail in tails for ci in cins]
        if tuple(t.shape) not in ok:
            raise ValueError(f"{n} must be {' or '.join(str(list(sh)) for sh in ok)}, got {tuple(t.shape)}")
        ins.append((n, t))
    c1 = cin - c0
    _check_half(H, W)
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    x1_shape = (B, L, c1 // 16, H, pitch, 16)

    def check(n, t):
        if n == "x1" and tuple(t.shape) != x1_shape:
            raise ValueError(f"out['x1'] {tuple(t.shape)} must match {lead_name} {tuple(lead.shape)}" +
                             (f" with {c1 // 16} planes" if entry.pass_channels else ""))
        if n == "x0" and (t.dim() != 6 or tuple(t.shape[:4]) != (B, L, c0 // 16, H0) or t.shape[4] < W0 or t.shape[5] != 16):
            raise ValueError(f"out['x0'] {tuple(t.shape)} must be [{B}, {L}, {c0 // 16}, {H0}, pitch0 >= {W0}, 16]")
        if t.data_ptr() % 16:
            raise ValueError(f"out['{n}'] must be 16-byte aligned")
    out = _outputs(out, want, dev, ins, check)
    pitch0 = int(given.shape[4]) if given is not None else V2ce3d._pitch(W0)
    shapes = {"x0": (B, L, c0 // 16, H0, pitch0, 16), "x1": x1_shape}
    detail = f"pitch {pitch}, pitch0 {pitch0}" + (f", {c0} + {c1} -> {cout}" if entry.pass_channels else "")
    res = _launch(entry, (c0, c1, cout), (B, L, H, W, pitch, pitch0), detail,
                  (hip.ptr(weight) if g1 is not None else None, hip.ptr(short_weight) if gd is not None else None, hip.ptr(g1),
                   hip.ptr(gd)), UPDGRAD_WANT, want, out, shapes, cap, dev)
    for n, t in res.items():
        t.lw, t.c16 = (W0 if n == "x0" else W), True
    return res


def convupn_dgrad(weight: Optional[torch.Tensor], short_weight: Optional[torch.Tensor], g1: Optional[torch.Tensor],
                  gd: Optional[torch.Tensor], *, want: Sequence[str] = UPDGRAD_WANT, out: Optional[dict] = None,
                  max_workgroups: int = 0, c0: Optional[int] = None) -> dict:
    """The gradients of the 3x3x3 and the 1x1x1 convolution c0 + c1 -> cout on the virtual tensor
    ``X = cat(nearest_upsample_2x(x0), x1)`` with respect to ``x0`` and ``x1`` (c0 = 64 or 128, c1 = 32 or 64, cout = 32 or
    64).  ``weight`` is the 3x3x3 convolution's own contiguous ``[cout, c0 + c1, 3, 3, 3]`` f32 weight, ``short_weight`` the
    1x1x1 convolution's ``[cout, c0 + c1]`` (or ``[cout, c0 + c1, 1, 1, 1]``); ``g1`` (the gradient with respect to the 3x3x3
    convolution's output) and ``gd`` (the gradient with respect to the 1x1x1 convolution's output) are channels-last-16
    ``[B, L, cout / 16, H, pitch, 16]`` f32 with the same shape and ``.lw``.  ``g1`` may be None (``weight`` is then
    unused): the 1x1x1 convolution's share alone; ``gd`` may be None (``short_weight`` likewise); not both.
    ``c0``: how the weight's input channels split.  96 is 64 + 32, 160 is 128 + 32 and 192 is 128 + 64, but 128 is 64 + 64
    or an ``x0`` of 128 channels with nothing beside it: a 128-channel weight is refused unless ``c0`` or ``out['x0']``
    (whose planes say it) is given.  Elsewhere ``c0`` may be omitted.
    -> {name: tensor} for the names in ``want`` (a subset of 'x0', 'x1'): 'x1' ``[B, L, c1 / 16, H, pitch, 16]`` = the last
    c1 channels of d_X = conv_transpose(g1, weight) + short_weight^T gd, 'x0' ``[B, L, c0 / 16, H0, pitch0, 16]`` with
    ``H0 = (H + 1) // 2``, ``.lw = (W + 1) // 2`` and ``pitch0 = V2ce3d._pitch(.lw)`` (or that of ``out['x0']``) = the first
    c0 channels summed over the output positions of each source pixel.  Both carry ``.lw`` and ``.c16``; their padding
    columns are zeros.  ``out``: {name: tensor} to write into.  ``max_workgroups``: 0 = the kernel's choice, n > 0 caps the
    grid (the bytes do not depend on n).  One call, no host synchronisation."""
    return _updgrad(_CONVUPN_DGRAD, weight, short_weight, g1, gd, want, out, max_workgroups, c0)


def convup_dgrad(weight: Optional[torch.Tensor], short_weight: Optional[torch.Tensor], g1: Optional[torch.Tensor],
                 gd: Optional[torch.Tensor], *, want: Sequence[str] = UPDGRAD_WANT, out: Optional[dict] = None,
                 max_workgroups: int = 0) -> dict:
    """``convupn_dgrad`` at 64 + 32 -> 32 through ``v2ce_convup_dgrad``: ``weight`` is ``[32, 96, 3, 3, 3]``,
    ``short_weight`` ``[32, 96]`` (or ``[32, 96, 1, 1, 1]``), ``g1``, ``gd`` and 'x1' are ``[B, L, 2, H, pitch, 16]`` and
    'x0' is ``[B, L, 4, H0, pitch0, 16]``; anything else is refused."""
    return _updgrad(_CONVUP_DGRAD, weight, short_weight, g1, gd, want, out, max_workgroups)
