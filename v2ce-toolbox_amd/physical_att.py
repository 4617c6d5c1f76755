"""Physical-attention maps, physical masks and log-frame residuals on the device: the reference's
``train/scripts/utils/physical_att.py``, from uint8 frames and the events between them.

* ``physical_mask_generation(events, frames, K, threshold=0.6, pool_size=8)``           :64-84    (mask, ratio_map)
* ``physical_attention_generation(events, frames, pool_size=8, ceiling=10)``            :107-146  float32 ``[Hp, Wp]``
* ``physical_attention_generation_advanced(events, frames, pool_size=8, ceiling=5)``    :150-193  float32 ``[Hp, Wp]``
* ``physical_attention_batch_generation(events, frames, pool_size=8, advanced, ceiling)`` :196-213  float32 ``[B, Hp, Wp]``
* ``gen_log_frame_residual(frames)`` / ``gen_log_frame_residual_batch(frames)``         :216-247  float32 ``[N-1, 1, H, W]``
* ``physical_attention_batch(frames, events, counts, ...)``  P frame pairs and their events in one call
* ``packet_physical_att(images, events, counts)``  the call of ``train/scripts/tools/gen_phy_att.py:25``
* ``main()``  the command line (``v2ce_prep.py``; ``--image_grad`` adds the image units of ``image_derivative``)

``Hp = ceil(H / pool_size)``, ``Wp = ceil(W / pool_size)`` (skimage's ``block_reduce`` pads with zeros).  Everything runs
``v2ce_physatt_batch`` / ``v2ce_log_residual_batch`` (``csrc/physatt.hip``), whose arithmetic follows NumPy's and SciPy's
operation by operation (``include/v2ce_hip.h``), so the maps carry the reference's bytes and are identical run to run.
``lin_log`` (``v2e_utils.py:5-43``) takes 256 arguments on uint8 frames: it is tabulated here on the host, with the
reference's own float64 formula, and looked up on the device.  There is no CPU path.

Deliberate differences from the reference:

* frames must be ``uint8``, or a float / integer array or tensor whose entries are all integers in [0, 255] (converted);
  anything else is a ``ValueError`` -- float-valued frames are not supported;
* inputs are never modified (the reference's ``lin_log`` adds 1e-8 into a float64 argument in place);
* the results are device tensors (the mask a ``torch.bool`` tensor);
* event coordinates outside ``W x H`` are a ``ValueError``, negative ones included (the reference wraps negative ones
  round as Python indices and raises ``IndexError`` on large ones); events arrive in the containers of
  ``event_grids`` (an ``[N, 4]`` float64 array only with integral entries);
* ``K`` outside ``[1, Hp * Wp]`` is a ``ValueError`` (the reference's ``K = 0`` selects every cell by accident);
* ``pool_size`` lies in [2, 16] and ``Hp * Wp`` within 6144 cells (260 x 346 from pool 4 on);
* a patch of 2^24 events or more is a ``ValueError`` (the reference's float32 sum of the count frame is not exact there).

As in the reference, ``physical_attention_batch_generation(advanced=False)`` ignores ``ceiling`` and uses 10.
"""
from __future__ import annotations

import argparse
import ctypes
import logging
import math
import os
import os.path as op
from typing import Tuple

import numpy as np
import torch

from . import hip
from .LDATI import DeviceEvents
from .event_grids import _columns, _device

logger = logging.getLogger("V2CE")

MODES = {"plain": hip.PHYSATT_PLAIN, "advanced": hip.PHYSATT_ADVANCED, "ratio": hip.PHYSATT_RATIO}
_LUTS = {}


def lin_log_lut(offset: float) -> np.ndarray:
    """float32 [256]: ``lin_log(v + offset)`` (v2e_utils.py:5-43, threshold 20) for the 256 values of a uint8 pixel, in the
    reference's float64 steps: ``x += 1e-8``, linear up to 20, ``round(y * 1e8) / 1e8``, cast to float32."""
    x = np.arange(256, dtype=np.float64) + offset
    f = (1.0 / 20) * math.log(20)
    x += 1e-8
    y = np.where(x <= 20, x * f, np.log(x))
    return (np.round(y * 1e8) / 1e8).astype(np.float32)


def gauss_weights() -> np.ndarray:
    """float64 [5]: the taps k = 0 .. 4 of ``scipy.ndimage.gaussian_filter(sigma=1)`` (radius 4), as SciPy forms them."""
    k = np.arange(-4, 5)
    phi = np.exp(-0.5 * k ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[4:])


def _lut(offset: float, dev: torch.device) -> torch.Tensor:
    key = (offset, str(dev))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(lin_log_lut(offset)).to(dev)
    return _LUTS[key]


def _frames_u8(frames, device) -> torch.Tensor:
    """Frames as a contiguous uint8 device tensor; host data is copied, never written."""
    if torch.is_tensor(frames):
        if not frames.is_cuda:
            raise hip.V2ceHipError(f"frames must live on a HIP device or be a host array (got a {frames.device} tensor); "
                                   "there is no CPU path")
        if frames.dtype != torch.uint8:
            f = frames.double() if frames.is_floating_point() else frames.long()
            if not bool(((f >= 0) & (f <= 255) & (f == f.floor())).all()):              # a synchronisation of its own
                raise ValueError("frames must hold integers in [0, 255] only; float-valued frames are not supported")
            frames = f.to(torch.uint8)
        return frames.contiguous()
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        if a.dtype.kind not in "fiub":
            raise ValueError(f"frames must be uint8 or a numeric array of integers in [0, 255], got {a.dtype}")
        with np.errstate(invalid="ignore"):
            ok = a.size == 0 or bool(np.all((a == np.floor(a)) & (a >= 0) & (a <= 255)))
        if not ok:
            raise ValueError("frames must hold integers in [0, 255] only; float-valued frames are not supported")
        a = a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).to(_device(device))


def _map_shape(H: int, W: int, pool_size: int) -> Tuple[int, int]:
    if not 2 <= pool_size <= 16:
        raise ValueError(f"pool_size must lie in [2, 16], got {pool_size}")
    return -(-H // pool_size), -(-W // pool_size)


def raise_for_status(status, what: str = "physical attention") -> None:
    """The exceptions of the drop-ins for the status words of ``physical_attention_batch`` (include/v2ce_hip.h)."""
    st = np.asarray(status).reshape(-1)
    where = lambda bit: np.flatnonzero(st & bit).tolist()[:10]
    if (st & hip.PHYSATT_BAD_OFFSETS).any():
        raise ValueError(f"{what}: the event offsets of pairs {where(hip.PHYSATT_BAD_OFFSETS)} do not ascend within the events")
    if (st & hip.PHYSATT_BAD_XY).any():
        raise ValueError(f"{what}: event coordinates outside the frame in pairs {where(hip.PHYSATT_BAD_XY)}")
    if (st & hip.PHYSATT_COUNT_OVERFLOW).any():
        raise ValueError(f"{what}: a patch of pairs {where(hip.PHYSATT_COUNT_OVERFLOW)} holds 2^24 events or more; the "
                         "reference's float32 count is not exact there")


def physical_attention_batch(frames, events, counts, pool_size: int = 8, mode: str = "advanced", ceiling=5,
                             threshold: float = 0.6, K: int = 0, device=None):
    """P frame pairs -> ``(maps, status)``, or ``(maps, masks, status)`` for ``mode="ratio"`` with ``K > 0``.

    ``frames``: a clip ``[P+1, H, W]`` (pair i = frames i, i + 1) or stacked pairs ``[P, 2, H, W]``, uint8 (host array or
    device tensor).  ``events``: the pairs' events back to back, in a container of ``event_grids`` (host structured array,
    integral ``[N, 4]`` float64 rows ``[timestamp, x, y, polarity]``, ``DeviceEvents`` -- ``counts=None`` takes its
    per-frame counts -- or a (ts, x, y, p) tuple of device tensors); ``counts`` [P] the events of each pair.
    ``mode``: ``"plain"`` / ``"advanced"`` (``physical_attention_generation`` / ``_advanced`` with ``ceiling``) or
    ``"ratio"`` (the ``ratio_map`` of ``physical_mask_generation`` with ``threshold``; ``K > 0`` adds the top-K masks).
    ``maps`` float32 ``[P, Hp, Wp]``, ``masks`` bool ``[P, Hp, Wp]``, ``status`` int32 [P] on the host (bits
    ``hip.PHYSATT_*``): a pair with a bit set got a zero map and does not disturb the others; ``raise_for_status``
    turns the words into exceptions.  One host synchronisation (the status)."""
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} (one of {tuple(MODES)})")
    pool_size, K = int(pool_size), int(K)
    if not torch.is_tensor(frames):
        frames = np.asarray(frames)
    shape = tuple(frames.shape)
    if len(shape) == 4 and shape[1] == 2:
        P, stride = shape[0], 2
    elif len(shape) == 3 and shape[0] >= 2:
        P, stride = shape[0] - 1, 1
    else:
        raise ValueError(f"frames must be a clip [P+1, H, W] or pairs [P, 2, H, W], got {shape}")
    H, W = int(shape[-2]), int(shape[-1])
    if P < 1 or H < 1 or W < 1:
        raise ValueError(f"no pairs or an empty frame: {shape}")
    Hp, Wp = _map_shape(H, W, pool_size)
    want_mask = mode == "ratio" and K != 0
    if mode == "ratio":
        if K != 0 and not 1 <= K <= Hp * Wp:
            raise ValueError(f"K must lie in [1, {Hp * Wp}] (the cells of the {Hp} x {Wp} map), got {K}")
        if not (float(threshold) > 0 and math.isfinite(float(threshold))):
            raise ValueError(f"threshold must be positive and finite, got {threshold}")
    elif not (float(ceiling) > 0 and math.isfinite(float(ceiling))):
        raise ValueError(f"ceiling must be positive and finite, got {ceiling}")
    if counts is None and isinstance(events, DeviceEvents):
        counts = events.frame_counts
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size != P:
        raise ValueError(f"{c.size} counts for {P} frame pairs")
    if (c < 0).any():
        raise ValueError("negative count")
    if int(c.sum()) != _length(events):
        raise ValueError(f"counts add up to {int(c.sum())}, the events are {_length(events)}")
    fr = _frames_u8(frames, device)
    dev = fr.device
    _, x, y, _ = _columns(events, dev, allow_rows=True)
    if x.device != dev:
        raise ValueError(f"frames live on {dev}, events on {x.device}")
    n = int(x.shape[0])
    L = hip.lib()
    ws_bytes = L.v2ce_physatt_workspace_bytes(P, H, W, pool_size, n)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"v2ce_physatt_batch: unsupported shape P={P}, H={H}, W={W}, pool_size={pool_size}, n={n} "
                               f"(the {Hp} x {Wp} map must fit 6144 cells)")
    gw = gauss_weights()
    with torch.cuda.device(dev):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        maps = torch.empty((P, Hp, Wp), dtype=torch.float32, device=dev)
        masks = torch.empty((P, Hp, Wp), dtype=torch.uint8, device=dev) if want_mask else None
        status = torch.empty(P, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        lut = _lut(1e-6, dev)
        hip.check(L.v2ce_physatt_batch(fr.data_ptr(), stride, P, H, W, x.data_ptr() if n else None,
                                       y.data_ptr() if n else None, off.data_ptr(), n, pool_size, MODES[mode],
                                       float(np.float32(ceiling)), float(np.float32(threshold)), K, lut.data_ptr(),
                                       gw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), maps.data_ptr(), hip.ptr(masks),
                                       status.data_ptr(), ws.data_ptr(), ws_bytes, hip.stream_ptr(dev)),
                  "v2ce_physatt_batch")
        st = status.cpu().numpy()                                   # the one synchronisation
    if want_mask:
        return maps, masks.bool(), st
    return maps, st


def _length(events) -> int:
    if isinstance(events, DeviceEvents):
        return events.num_events
    if isinstance(events, (tuple, list)) and len(events) == 4 and all(torch.is_tensor(e) for e in events):
        return int(events[0].shape[0])
    return len(events)


def _pair(frames):
    if tuple(frames.shape[:1]) != (2,) or len(frames.shape) != 3:
        raise ValueError(f"frames must be one pair [2, H, W], got {tuple(frames.shape)}")
    return frames


def physical_mask_generation(events, frames, K, threshold=0.6, pool_size=8, device=None):
    """physical_att.py:64-84: ``(mask, ratio_map)``, bool and float32 ``[Hp, Wp]`` device tensors; the mask marks the
    cells at or above the K-th largest ratio (more than K on a tie).  Deviation: ``K`` outside ``[1, Hp * Wp]`` raises."""
    Hp, Wp = _map_shape(int(frames.shape[-2]), int(frames.shape[-1]), int(pool_size))
    if not 1 <= int(K) <= Hp * Wp:
        raise ValueError(f"K must lie in [1, {Hp * Wp}] (the cells of the {Hp} x {Wp} map), got {K}")
    maps, masks, st = physical_attention_batch(_pair(frames), events, [_length(events)], pool_size, "ratio",
                                               threshold=threshold, K=K, device=device)
    raise_for_status(st, "physical_mask_generation")
    return masks[0], maps[0]


def physical_attention_generation(events, frames, pool_size=8, ceiling=10, device=None):
    """physical_att.py:107-146: float32 ``[Hp, Wp]`` on the device, the clipped and blurred ratio over ``ceiling``."""
    maps, st = physical_attention_batch(_pair(frames), events, [_length(events)], pool_size, "plain", ceiling=ceiling,
                                        device=device)
    raise_for_status(st, "physical_attention_generation")
    return maps[0]


def physical_attention_generation_advanced(events, frames, pool_size=8, ceiling=5, device=None):
    """physical_att.py:150-193: float32 ``[Hp, Wp]`` on the device, the clipped and blurred ratio stretched to [0, 1]."""
    maps, st = physical_attention_batch(_pair(frames), events, [_length(events)], pool_size, "advanced", ceiling=ceiling,
                                        device=device)
    raise_for_status(st, "physical_attention_generation_advanced")
    return maps[0]


def physical_attention_batch_generation(events, frames, pool_size=8, advanced=False, ceiling=5, device=None):
    """physical_att.py:196-213: ``events`` a list of B event containers, ``frames`` ``[B, 2, H, W]``; float32
    ``[B, Hp, Wp]`` on the device, all pairs in one call.  As in the reference, ``advanced=False`` ignores ``ceiling``
    and uses the default 10 of ``physical_attention_generation``."""
    B = int(frames.shape[0])
    if len(events) != B:
        raise ValueError(f"{len(events)} event lists for {B} frame pairs")
    fr = _frames_u8(frames, device)
    cols = [_columns(e, fr.device, allow_rows=True) for e in events]
    joined = tuple(torch.cat([c[k] for c in cols]) for k in range(4))
    maps, st = physical_attention_batch(fr, joined, [int(c[0].shape[0]) for c in cols], pool_size,
                                        "advanced" if advanced else "plain", ceiling=ceiling if advanced else 10)
    raise_for_status(st, "physical_attention_batch_generation")
    return maps


def packet_physical_att(images, events, counts, device=None):
    """The call of ``train/scripts/tools/gen_phy_att.py:25`` on one packet: ``images`` ``[L+1, H, W]`` uint8, the events
    of its L pairs back to back with ``counts`` [L]; pool 8, advanced, ceiling 25.  float32 ``[L, Hp, Wp]`` on the device."""
    maps, st = physical_attention_batch(images, events, counts, 8, "advanced", ceiling=25, device=device)
    raise_for_status(st, "packet_physical_att")
    return maps


def gen_log_frame_residual_batch(frames, device=None) -> torch.Tensor:
    """physical_att.py:232-247: ``lin_log(frames[1:]) - lin_log(frames[:-1])``, float32 ``[N-1, 1, H, W]`` on the device
    from uint8 ``[N, H, W]`` (the residual of ``EventPackDataset.__getitem__``)."""
    if len(frames.shape) != 3 or frames.shape[0] < 2:
        raise ValueError(f"frames must be [N, H, W] with N >= 2, got {tuple(frames.shape)}")
    fr = _frames_u8(frames, device)
    N, H, W = (int(s) for s in fr.shape)
    if H < 1 or W < 1:
        raise ValueError(f"empty frames: {tuple(fr.shape)}")
    dev = fr.device
    with torch.cuda.device(dev):
        out = torch.empty((N - 1, 1, H, W), dtype=torch.float32, device=dev)
        hip.check(hip.lib().v2ce_log_residual_batch(fr.data_ptr(), N, H, W, _lut(0.0, dev).data_ptr(), out.data_ptr(),
                                                    hip.stream_ptr(dev)), "v2ce_log_residual_batch")
    return out


def gen_log_frame_residual(frames, device=None) -> torch.Tensor:
    """physical_att.py:216-230: one pair ``[2, H, W]`` -> float32 ``[1, H, W]`` on the device."""
    return gen_log_frame_residual_batch(_pair(frames), device)[0]


# ---------------------------------------------------------------------------------------------------------------------
# command line (v2ce_prep.py)

def build_parser():
    p = argparse.ArgumentParser(description="Physical-attention maps and log-frame residuals of a recording "
                                            "(physical_att.py), one per frame pair")
    p.add_argument("--frames", type=str, required=True, help="the clip: uint8 [N, H, W] (.npy)")
    p.add_argument("--events", type=str, required=True,
                   help="events: .npz with key event_stream, or a structured .npy (timestamp, x, y, polarity)")
    p.add_argument("--frame_timestamps", type=str, help="int64 us frame times [N] (.npy): pair i is [T_i, T_i+1)")
    p.add_argument("--fps", type=float, default=None, help="without --frame_timestamps: T_i = int(i * 1 / fps * 1e6)")
    p.add_argument("--pool", type=int, default=8)
    p.add_argument("--ceiling", type=float, default=25)
    p.add_argument("--mode", type=str, default="advanced", choices=["plain", "advanced"])
    p.add_argument("--chunk", type=int, default=64, help="frame pairs per device call")
    p.add_argument("--image_grad", action="store_true",
                   help="also write the three-channel image units of --apply_image_grad (image_units.npy, image_grad_max.npy)")
    p.add_argument("--seq_len", type=int, default=16, help="with --image_grad: frame pairs per packet (the gradient channel "
                                                           "is normalised by its packet's maximum); whole packets of "
                                                           "about --chunk pairs go through the device at a time")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("-o", "--out_folder", type=str, default="./results")
    p.add_argument("-l", "--log_level", type=str, default="info")
    return p


def main(argv=None):
    """Writes ``physical_att.npy`` float32 [N-1, Hp, Wp], ``lfr.npy`` float32 [N-1, 1, H, W] and ``status.npy`` (int32 per
    pair).  A pair with coordinates outside the frame stops the command.  With ``--image_grad`` also ``image_units.npy``
    float32 [N-1, 3, H, W] and ``image_grad_max.npy`` float32 [ceil((N-1) / seq_len)] (``image_derivative.clip_image_units``)."""
    from . import glue
    from .stage2_metrics import load_events, split_by_frames
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()))
    dev = torch.device(args.device)
    if dev.type == "cuda" and dev.index is not None:
        torch.cuda.set_device(dev)
    clip = np.load(args.frames, allow_pickle=False)
    if clip.ndim != 3 or clip.shape[0] < 2:
        raise SystemExit(f"--frames must hold [N, H, W] with N >= 2, got {clip.shape}")
    N = clip.shape[0]
    ev = load_events(args.events)
    if args.frame_timestamps is not None:
        T = np.load(args.frame_timestamps).astype(np.int64).reshape(-1)
    elif args.fps is not None:
        T = np.asarray([glue.frame_offset_us(i, args.fps) for i in range(N)], dtype=np.int64)
    else:
        raise SystemExit("need --frame_timestamps or --fps")
    if T.size != N:
        raise SystemExit(f"{T.size} frame timestamps for {N} frames")
    ev, counts, dropped = split_by_frames(ev, T)
    logger.info(f"{len(ev)} events in {counts.size} pairs; {dropped} outside the frame times dropped")
    frames = _frames_u8(clip, dev)
    maps, lfr, status = [], [], []
    lo = 0
    for c0 in range(0, N - 1, args.chunk):
        c = counts[c0:c0 + args.chunk]
        hi = lo + int(c.sum())
        part = frames[c0:c0 + c.size + 1]
        m, st = physical_attention_batch(part, ev[lo:hi], c, args.pool, args.mode, ceiling=args.ceiling, device=dev)
        raise_for_status(st, f"pairs from {c0}")
        maps.append(m.cpu().numpy())
        lfr.append(gen_log_frame_residual_batch(part).cpu().numpy())
        status.append(st)
        lo = hi
    os.makedirs(args.out_folder, exist_ok=True)
    for name, parts in (("physical_att", maps), ("lfr", lfr), ("status", status)):
        np.save(op.join(args.out_folder, f"{name}.npy"), np.concatenate(parts))
        print(op.join(args.out_folder, f"{name}.npy"))
    if args.image_grad:
        from .image_derivative import clip_image_units
        if args.seq_len < 1:
            raise SystemExit(f"--seq_len must be positive, got {args.seq_len}")
        # whole packets per device call, about --chunk pairs: the device holds one piece's units at a time
        step = max(1, args.chunk // args.seq_len) * args.seq_len
        units, gmax = [], []
        for c0 in range(0, N - 1, step):
            u, g = clip_image_units(frames[c0:c0 + step + 1], seq_len=args.seq_len)
            units.append(u.cpu().numpy())
            gmax.append(g.cpu().numpy())
        for name, parts in (("image_units", units), ("image_grad_max", gmax)):
            np.save(op.join(args.out_folder, f"{name}.npy"), np.concatenate(parts))
            print(op.join(args.out_folder, f"{name}.npy"))


if __name__ == "__main__":
    main()
