"""The image-gradient input channel on the device: the reference's ``train/scripts/utils/image_derivative.py`` and the
three-channel ``image_units`` of ``EventPackDataset`` (``train/scripts/data/event_pack_dataset.py:66-75``), from uint8
frames.

* ``get_batch_double_blurred_image_gradient(image1, image2, sigma=3, kernel_size=11)``  :38-56   float32 ``[b, 1, h, w]``
* ``batch_img_gradient(img)``                                                          :58-75   float32 ``[b, c, h, w]``
* ``batch_img_residual(img1, img2)``                                                   :77-87   float32 ``[b, c, h, w]``
* ``image_units_batch(frames, seq_len=None, mean, std, sigma, kernel_size, apply_image_grad=True)``  S packets in one
  call: ``(units [S, L, 3, H, W], gmax [S])``, what a model built with ``--apply_image_grad`` consumes

Everything runs ``v2ce_image_grad_batch`` / ``v2ce_image_units_grad`` (``csrc/imgrad.hip``; the arithmetic is stated in
``include/v2ce_hip.h``).  There is no CPU path.

Deliberate differences from the reference:

* the Sobel sums are taken on the uint8 pixels as integers and the blur is two 1-D passes, so channel 2 is closer to the
  exact value of the formula than the reference's two float32 convolutions, not byte-equal to them (tests/image_grad_ref.py
  is the float64 statement; the goldens record the reference's own error);
* frames must be ``uint8`` (or another integer type within [0, 255]), or the reference's ``/ 255`` float tensors whose
  entries are all ``k / 255`` (converted back through ``round(x * 255)``); anything else is a ``ValueError`` --
  float-valued frames are not supported, as in ``physical_att``;
* ``kernel_size`` is odd and lies in [3, 15], ``sigma > 0``; ``h`` or ``w`` below ``kernel_size // 2 + 1`` is a
  ``ValueError`` (the reference's reflect pad raises there);
* the results are device tensors;
* ``batch_img_gradient`` needs ``h, w >= 2`` (it runs the blur kernel with the taps (0, 1, 0), which is the identity).

Out of scope: the NumPy / SciPy forms ``get_image_gradient`` and ``get_double_blurred_image_gradient`` (called nowhere in
the reference) and ``batch_image_derivative_calc`` / ``single_image_derivative_calc`` (they need an optical-flow network).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import hip
from .event_grids import _device

MAX_KERNEL_SIZE = 15
_NOT_K255 = ("float frames must hold k / 255 for integers k in [0, 255] only (the reference's uint8 frames / 255); "
             "float-valued frames are not supported")
_TABLES = {}


def gaussian_taps(kernel_size: int = 11, sigma: float = 3) -> np.ndarray:
    """float32 [kernel_size]: torchvision's ``_get_gaussian_kernel1d`` in its own steps, torch float32 on the CPU:
    ``linspace(-(k-1)/2, (k-1)/2, k)``, ``exp(-0.5 (x / sigma)^2)``, divided by its sum."""
    kernel_size = int(kernel_size)
    if kernel_size % 2 == 0 or not 3 <= kernel_size <= MAX_KERNEL_SIZE:
        raise ValueError(f"kernel_size must be odd and lie in [3, {MAX_KERNEL_SIZE}], got {kernel_size}")
    if not (float(sigma) > 0 and np.isfinite(float(sigma))):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    return np.ascontiguousarray((pdf / pdf.sum()).numpy().astype(np.float32))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _frames_u8(frames, device) -> torch.Tensor:
    """Frames as a contiguous uint8 device tensor: uint8 / integers in [0, 255] as they are, floats only when every entry
    is ``k / 255`` (a synchronisation of its own); host data is copied, never written."""
    if not torch.is_tensor(frames):
        a = np.asarray(frames)
        if a.dtype.kind not in "fiu":
            raise ValueError(f"frames must be uint8, integers in [0, 255] or k / 255 floats, got {a.dtype}")
        if a.dtype.kind == "f":
            with np.errstate(invalid="ignore"):
                k = np.nan_to_num(np.clip(np.round(a.astype(np.float64) * 255), 0, 255)).astype(np.int64)
            div = (lambda v: v / 255.0) if a.dtype == np.float64 else (lambda v: (v.astype(np.float32) / np.float32(255)).astype(a.dtype))
            if not np.array_equal(div(k), a):
                raise ValueError(_NOT_K255)
            a = k
        elif a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("integer frames must lie in [0, 255]")
        return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8))).to(_device(device))
    if not frames.is_cuda:
        raise hip.V2ceHipError(f"frames must live on a HIP device or be a host array (got a {frames.device} tensor); "
                               "there is no CPU path")
    if frames.dtype == torch.uint8:
        return frames.contiguous()
    if frames.is_floating_point():
        # k / 255 as the host divides it (a device division by a scalar may multiply by the reciprocal instead)
        table = np.arange(256, dtype=np.float64) / 255.0 if frames.dtype == torch.float64 else \
            np.arange(256, dtype=np.float32) / np.float32(255)
        table = torch.from_numpy(table).to(frames.device).to(frames.dtype)
        k = torch.round(frames.double() * 255).clamp(0, 255)
        k = torch.where(torch.isnan(k), torch.zeros_like(k), k)
        if not bool((table[k.long()] == frames).all()):
            raise ValueError(_NOT_K255)
    elif frames.dtype == torch.bool:
        raise ValueError("frames must be uint8, integers in [0, 255] or k / 255 floats, got bool")
    else:
        k = frames
        if not bool(((k >= 0) & (k <= 255)).all()):
            raise ValueError("integer frames must lie in [0, 255]")
    return k.to(torch.uint8).contiguous()


def _check_size(H: int, W: int, kernel_size: int) -> None:
    r = kernel_size // 2
    if H < r + 1 or W < r + 1:
        raise ValueError(f"frames of {H} x {W} are smaller than kernel_size // 2 + 1 = {r + 1}: the reflect padding of the "
                         "blur does not exist there")


def _grad_batch(fr: torch.Tensor, taps: np.ndarray):
    """uint8 ``[S, L+1, H, W]`` on the device -> ``(blur [S, L, H, W], gmax [S])``."""
    S, L1, H, W = (int(s) for s in fr.shape)
    _check_size(H, W, taps.size)
    dev = fr.device
    with torch.cuda.device(dev):
        blur = torch.empty((S, L1 - 1, H, W), dtype=torch.float32, device=dev)
        gmax = torch.empty(S, dtype=torch.float32, device=dev)
        hip.check(hip.lib().v2ce_image_grad_batch(fr.data_ptr(), S, L1 - 1, H, W, _fp(taps), taps.size, blur.data_ptr(),
                                                  gmax.data_ptr(), hip.stream_ptr(dev)), "v2ce_image_grad_batch")
    return blur, gmax


def _shape(x) -> tuple:
    """The shape of a tensor, an array or anything ``np.asarray`` takes (a list, a scalar)."""
    return tuple(x.shape) if torch.is_tensor(x) else np.shape(x)


def _pairs_u8(image1, image2, device) -> torch.Tensor:
    """Two non-empty ``[b, 1, h, w]`` inputs -> uint8 ``[b, 2, h, w]`` on the device."""
    s1, s2 = _shape(image1), _shape(image2)
    if s1 != s2 or len(s1) != 4 or s1[1] != 1 or 0 in s1:
        raise ValueError(f"image1 and image2 must both be a non-empty [b, 1, h, w], got {s1} and {s2}")
    a = _frames_u8(image1, device)
    b = _frames_u8(image2, a.device)
    return torch.cat([a, b], dim=1)


def get_batch_double_blurred_image_gradient(image1, image2, sigma=3, kernel_size=11, device=None) -> torch.Tensor:
    """image_derivative.py:38-56: the point-wise maximum of the two frames' Sobel magnitudes, blurred; float32
    ``[b, 1, h, w]`` on the device from two ``[b, 1, h, w]`` inputs (uint8, or the reference's ``/ 255`` floats)."""
    taps = gaussian_taps(kernel_size, sigma)
    blur, _ = _grad_batch(_pairs_u8(image1, image2, device), taps)
    return blur


def batch_img_gradient(img, device=None) -> torch.Tensor:
    """image_derivative.py:58-75: the Sobel magnitude of zero-padded frames, float32 ``[b, c, h, w]`` on the device (the
    reference itself runs for ``c = 1`` only; every channel is treated alike here)."""
    if len(_shape(img)) != 4 or 0 in _shape(img):
        raise ValueError(f"img must be a non-empty [b, c, h, w], got {_shape(img)}")
    fr = _frames_u8(img, device)
    b, c, h, w = (int(s) for s in fr.shape)
    pairs = fr.reshape(b * c, 1, h, w).expand(b * c, 2, h, w).contiguous()
    blur, _ = _grad_batch(pairs, np.asarray([0, 1, 0], dtype=np.float32))          # identity taps: the gradient itself
    return blur.reshape(b, c, h, w)


def batch_img_residual(img1, img2, device=None) -> torch.Tensor:
    """image_derivative.py:77-87: ``img2 - img1`` of the ``/ 255`` frames, float32 ``[b, c, h, w]`` on the device:
    ``v2ce_log_residual_batch`` with the table ``k / 255`` on the two batches as the two frames of one tall pair."""
    s1, s2 = _shape(img1), _shape(img2)
    if s1 != s2 or len(s1) != 4 or 0 in s1:
        raise ValueError(f"img1 and img2 must both be a non-empty [b, c, h, w], got {s1} and {s2}")
    a = _frames_u8(img1, device)
    b = _frames_u8(img2, a.device)
    n, c, h, w = (int(s) for s in a.shape)
    rows = n * c * h
    if rows >= 1 << 31:
        raise hip.V2ceHipError(f"batch_img_residual: {rows} rows exceed the kernel's int32 frame height")
    dev = a.device
    pair = torch.stack([a, b])                                     # [2, b, c, h, w] = two frames of b * c * h rows
    key = ("k/255", str(dev))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(dev)
    with torch.cuda.device(dev):
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
        hip.check(hip.lib().v2ce_log_residual_batch(pair.data_ptr(), 2, rows, w, _TABLES[key].data_ptr(), out.data_ptr(),
                                                    hip.stream_ptr(dev)), "v2ce_log_residual_batch")
    return out


def image_units_batch(frames, seq_len=None, mean=0.153, std=0.165, sigma=3, kernel_size=11, apply_image_grad=True,
                      device=None):
    """The ``image_units`` of ``EventPackDataset.__getitem__`` (event_pack_dataset.py:66-75) for S packets in one call.

    ``frames``: uint8 ``[S, L+1, H, W]`` (packet s = L pairs of consecutive frames), or a clip ``[N, H, W]``: one packet of
    ``N - 1`` pairs, or with ``seq_len`` the packets of ``seq_len`` pairs each (packet s = frames ``s * seq_len`` to
    ``(s + 1) * seq_len``; ``N - 1`` must be a multiple).  Returns ``(units, gmax)``: float32 ``[S, L, 3, H, W]`` --
    channels 0 / 1 the normalised frames of a pair, channel 2 the blurred gradient over its packet's maximum -- and the
    maxima float32 ``[S]``, both on the device.  ``apply_image_grad=False``: ``units`` ``[S, L, 2, H, W]`` (:75), ``gmax``
    None.  With ``apply_image_grad=True`` uint8 device frames make one library call and no host synchronisation; the
    two-channel form makes one ``v2ce_preprocess_pairs`` launch per packet (S launches, no synchronisation either)."""
    if len(_shape(frames)) not in (3, 4):
        raise ValueError(f"frames must be [S, L+1, H, W] or a clip [N, H, W], got {_shape(frames)}")
    fr = _frames_u8(frames, device)
    if fr.dim() == 3:
        N = int(fr.shape[0])
        if seq_len is None:
            fr = fr[None]
        else:
            seq_len = int(seq_len)
            if seq_len < 1 or N < 2 or (N - 1) % seq_len:
                raise ValueError(f"a clip of {N} frames does not split into packets of {seq_len} pairs")
            idx = torch.arange(0, N - 1, seq_len, device=fr.device)[:, None] + torch.arange(seq_len + 1, device=fr.device)
            fr = fr[idx]
    elif seq_len is not None and int(seq_len) != int(fr.shape[1]) - 1:
        raise ValueError(f"seq_len = {seq_len} does not match frames of {tuple(fr.shape)}")
    fr = fr.contiguous()
    S, L1, H, W = (int(s) for s in fr.shape)
    if S < 1 or L1 < 2 or H < 1 or W < 1:
        raise ValueError(f"no pairs or an empty frame: {tuple(fr.shape)}")
    L = L1 - 1
    dev = fr.device
    lib = hip.lib()
    mean, std = float(np.float32(mean)), float(np.float32(std))
    if not apply_image_grad:
        with torch.cuda.device(dev):
            units = torch.empty((S, L, 2, H, W), dtype=torch.float32, device=dev)
            for s in range(S):
                hip.check(lib.v2ce_preprocess_pairs(fr[s].data_ptr(), L1, H, W, mean, std, units[s].data_ptr(),
                                                    hip.stream_ptr(dev)), "v2ce_preprocess_pairs")
        return units, None
    taps = gaussian_taps(kernel_size, sigma)
    _check_size(H, W, taps.size)
    ws_bytes = lib.v2ce_image_grad_workspace_bytes(S, L, H, W)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"v2ce_image_units_grad: unsupported shape S={S}, L={L}, H={H}, W={W}")
    with torch.cuda.device(dev):
        units = torch.empty((S, L, 3, H, W), dtype=torch.float32, device=dev)
        gmax = torch.empty(S, dtype=torch.float32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        hip.check(lib.v2ce_image_units_grad(fr.data_ptr(), S, L, H, W, _fp(taps), taps.size, mean, std, units.data_ptr(),
                                            gmax.data_ptr(), ws.data_ptr(), ws_bytes, hip.stream_ptr(dev)),
                  "v2ce_image_units_grad")
    return units, gmax


def clip_image_units(frames, seq_len=16, device=None, **kw):
    """A clip ``[N, H, W]`` cut like the dataset's packets, the last one as short as the clip leaves it:
    ``(units [N-1, 3, H, W], gmax [ceil((N-1) / seq_len)])`` (``v2ce_prep.py --image_grad``)."""
    fr = _frames_u8(frames, device)
    if fr.dim() != 3 or fr.shape[0] < 2:
        raise ValueError(f"frames must be [N, H, W] with N >= 2, got {tuple(fr.shape)}")
    seq_len = int(seq_len)
    if seq_len < 1:
        raise ValueError(f"seq_len must be positive, got {seq_len}")
    pairs = int(fr.shape[0]) - 1
    full = pairs - pairs % seq_len
    units, gmax = [], []
    if full:
        u, g = image_units_batch(fr[:full + 1], seq_len=seq_len, **kw)
        units.append(u.reshape(full, *u.shape[2:]))
        gmax.append(g)
    if pairs > full:
        u, g = image_units_batch(fr[full:], **kw)
        units.append(u[0])
        gmax.append(g)
    return torch.cat(units), torch.cat(gmax)
