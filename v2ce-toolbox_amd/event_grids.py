"""Events -> signed, split and statistics voxel grids on the device: the three encoders that stand next to
``gen_discretized_event_volume`` (``voxelize.py``) in ``train/scripts/utils/events_utils.py``.

* ``events_to_voxel_grid(events, num_bins, width, height)``             :70-116   float32 ``[bins, H, W]``
* ``structured_events_to_voxel_grid(events, num_bins, width, height)``  :215-260  float32 ``[2, bins, H, W]``
* ``structured_events_to_voxel_stat(events, num_bins, width, height)``  :333-358  three float64 ``[2, bins, H, W]``
* ``event_grids_batch(events, counts, bins, H, W, kinds)``  many event lists (frame pairs) in one call
* ``main()``  the command line (``v2ce_encode.py``)

All of them run ``v2ce_event_grids_batch`` (``csrc/voxelize.hip``): one bucketing of the events by (list, pixel) feeds
every requested kind, each cell is summed in the order and with the roundings of the reference's ``np.add.at`` calls,
so the grids carry the reference's bytes and are identical run to run.  There is no CPU path.

Deliberate differences from the reference:

* the input is never modified (the reference rescales the timestamp column of an ``[N, 4]`` array in place, rewrites
  polarity 0 as -1 in the grid encoders and -1 as 0 in the stat encoder);
* the results are device tensors;
* an ``[N, 4]`` float array is taken by ``events_to_voxel_grid`` only if every entry is integral and the polarity column
  holds -1, 0 or 1 (the device columns are int64 / int16 / int8); anything else is a ``ValueError``, where the reference
  would interpolate fractional timestamps and truncate fractional coordinates;
* coordinates outside ``width x height`` and timestamps outside ``[first, last]`` of their list (an unsorted list) are a
  ``ValueError``: the reference then writes to a wrapped-around cell or raises, depending on the value;
* the stat encoder raises ``ValueError`` when a cell's sum of squared residues reaches 2^53, where the reference's float64
  sum starts to depend on the order of its adds.
"""
from __future__ import annotations

import argparse
import logging
import os
import os.path as op
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .LDATI import DeviceEvents

logger = logging.getLogger("V2CE")

KINDS = {"signed": hip.EVENT_GRIDS_SIGNED, "split": hip.EVENT_GRIDS_SPLIT, "stat": hip.EVENT_GRIDS_STAT}
_FIELDS = (("timestamp", np.int64, torch.int64), ("x", np.int16, torch.int16), ("y", np.int16, torch.int16),
           ("polarity", np.int8, torch.int8))


def _device(device):
    if device is not None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise hip.V2ceHipError(f"device {dev} is not a HIP device; there is no CPU path")
        return dev
    if not torch.cuda.is_available():
        raise hip.V2ceHipError("no HIP device is available; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _from_float_rows(ev: np.ndarray):
    """An [N, 4] float array [timestamp, x, y, polarity] (events_utils.py:74) as integer columns."""
    if ev.ndim != 2 or ev.shape[1] != 4:
        raise ValueError(f"an unstructured event array must be [N, 4], got {ev.shape}")
    if ev.dtype != np.float64:
        raise ValueError(f"an unstructured event array must be float64, got {ev.dtype}")
    if not np.isfinite(ev).all() or (ev != np.trunc(ev)).any():
        raise ValueError("an [N, 4] event array must hold integral values only (timestamps in whole microseconds, "
                         "pixel coordinates); fractional entries are not supported")
    if not np.isin(ev[:, 3], (-1.0, 0.0, 1.0)).all():
        raise ValueError("the polarity column of an [N, 4] event array must hold -1, 0 or 1")
    if ev.shape[0] and (np.abs(ev[:, 1:3]).max() > 32767 or np.abs(ev[:, 0]).max() >= 2.0 ** 53):
        raise ValueError("an [N, 4] event array holds a coordinate beyond int16 or a timestamp beyond 2^53")
    return [ev[:, k].astype(dt) for k, (_, dt, _) in enumerate(_FIELDS)]


def _columns(events, device, allow_rows: bool):
    """Events as (ts int64, x int16, y int16, p int8) device tensors; host data is copied, never written."""
    if isinstance(events, DeviceEvents):
        return tuple(events._unpacked())
    if isinstance(events, torch.Tensor):
        if not events.is_cuda:
            raise hip.V2ceHipError(f"events must live on a HIP device (got {events.device}); there is no CPU path")
        raise TypeError("a single tensor is not an event container: pass a (ts, x, y, p) tuple of device tensors")
    if isinstance(events, (tuple, list)) and len(events) == 4 and all(torch.is_tensor(e) for e in events):
        for t, (name, _, dt) in zip(events, _FIELDS):
            if not t.is_cuda:
                raise hip.V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
            if t.dtype != dt or not t.is_contiguous() or t.dim() != 1:
                raise TypeError(f"{name} must be a contiguous 1-d {dt} tensor")
        if len({int(t.shape[0]) for t in events}) != 1:
            raise ValueError("the event columns differ in length")
        return tuple(events)
    ev = np.asarray(events)
    if ev.dtype.names is None:
        if not allow_rows:
            raise TypeError("events must be a structured array with fields timestamp, x, y, polarity (the LDATI record "
                            "dtype), a DeviceEvents or a (ts, x, y, p) tuple of device tensors")
        cols = _from_float_rows(ev)
    else:
        if not {"timestamp", "x", "y", "polarity"} <= set(ev.dtype.names):
            raise TypeError("a structured event array needs the fields timestamp, x, y, polarity")
        cols = [np.array(ev[f], dtype=dt) for f, dt, _ in _FIELDS]          # fresh, packed copies of the fields
    dev = _device(device)
    return tuple(torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols)


def _kind_mask(kinds) -> int:
    if isinstance(kinds, str):
        kinds = (kinds,)
    mask = 0
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"unknown kind {k!r} (one of {tuple(KINDS)})")
        mask |= KINDS[k]
    if not mask:
        raise ValueError("no kind requested")
    return mask


def raise_for_status(status, what: str = "event grids") -> None:
    """The exceptions of the drop-ins for the status words of ``event_grids_batch`` (include/v2ce_hip.h)."""
    st = np.asarray(status).reshape(-1)
    where = lambda bit: np.flatnonzero(st & bit).tolist()[:10]
    if (st & hip.EVENT_GRIDS_EMPTY).any():
        raise IndexError(f"{what}: no events in lists {where(hip.EVENT_GRIDS_EMPTY)} (the reference raises on events[-1])")
    if (st & hip.EVENT_GRIDS_BAD_XY).any():
        raise ValueError(f"{what}: event coordinates outside the grid in lists {where(hip.EVENT_GRIDS_BAD_XY)}")
    if (st & hip.EVENT_GRIDS_BAD_TIME).any():
        raise ValueError(f"{what}: a timestamp outside [first, last] of its list (unsorted events) in lists "
                         f"{where(hip.EVENT_GRIDS_BAD_TIME)}")
    if (st & hip.EVENT_GRIDS_STAT_TOP_EDGE).any():
        raise IndexError(f"{what}: the last timestamp falls into bin num_bins (last - first is a multiple of num_bins) in "
                         f"lists {where(hip.EVENT_GRIDS_STAT_TOP_EDGE)}; the reference raises IndexError here")
    if (st & hip.EVENT_GRIDS_STAT_OVERFLOW).any():
        raise ValueError(f"{what}: a cell's sum of squared time residues reached 2^53 in lists "
                         f"{where(hip.EVENT_GRIDS_STAT_OVERFLOW)}; the reference's float64 sum is not exact there")


def event_grids_batch(events, counts, bins: int, H: int, W: int, kinds: Sequence[str] = ("signed", "split", "stat"),
                      device=None) -> Tuple[Dict[str, torch.Tensor], np.ndarray]:
    """P event lists -> ``(grids, status)``.

    ``events``: the lists back to back as a host structured array (fields timestamp, x, y, polarity), a ``DeviceEvents``
    (``counts=None`` takes its per-frame counts) or a (ts, x, y, p) tuple of device tensors; ``counts`` [P] the length
    of each list.  ``grids`` holds, per requested kind, device tensors with the list axis first: ``"signed"`` f32
    [P, bins, H, W]; ``"split"`` f32 [P, 2, bins, H, W]; ``"stat_count"``, ``"stat_mean"``, ``"stat_std"`` f64
    [P, 2, bins, H, W].  ``status`` int32 [P] (bits ``hip.EVENT_GRIDS_*``): a list with a bit set got zero grids (a
    stat-only bit zeroes the stat grids only) and does not disturb the others; ``raise_for_status`` turns the words
    into the exceptions of the drop-ins.  ``bins`` in [1, 16].  One host synchronisation (the status)."""
    bins, H, W = int(bins), int(H), int(W)
    mask = _kind_mask(kinds)
    if not 1 <= bins <= 16:
        raise ValueError(f"bins must lie in [1, 16], got {bins}")
    if H < 1 or W < 1:
        raise ValueError(f"height and width must be positive, got {H} x {W}")
    if counts is None and isinstance(events, DeviceEvents):
        counts = events.frame_counts
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    P = c.size
    if P == 0:
        raise ValueError("no lists")
    if (c < 0).any():
        raise ValueError("negative count")
    ts, x, y, p = _columns(events, device, allow_rows=True)
    dev = ts.device
    n = int(ts.shape[0])
    if int(c.sum()) != n:
        raise ValueError(f"counts add up to {int(c.sum())}, the events are {n}")
    L = hip.lib()
    ws_bytes = L.v2ce_event_grids_workspace_bytes(P, bins, H, W, n, mask)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"v2ce_event_grids_batch: unsupported shape P={P}, bins={bins}, H={H}, W={W}, n={n}")
    out: Dict[str, torch.Tensor] = {}
    with torch.cuda.device(dev):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        if mask & hip.EVENT_GRIDS_SIGNED:
            out["signed"] = torch.empty((P, bins, H, W), dtype=torch.float32, device=dev)
        if mask & hip.EVENT_GRIDS_SPLIT:
            out["split"] = torch.empty((P, 2, bins, H, W), dtype=torch.float32, device=dev)
        if mask & hip.EVENT_GRIDS_STAT:
            for k in ("stat_count", "stat_mean", "stat_std"):
                out[k] = torch.empty((P, 2, bins, H, W), dtype=torch.float64, device=dev)
        status = torch.empty(P, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if n else None
        optr = lambda k: out[k].data_ptr() if k in out else None
        hip.check(L.v2ce_event_grids_batch(ptr(ts), ptr(x), ptr(y), ptr(p), off.data_ptr(), n, P, bins, H, W, mask,
                                           optr("signed"), optr("split"), optr("stat_count"), optr("stat_mean"),
                                           optr("stat_std"), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                           hip.stream_ptr(dev)), "v2ce_event_grids_batch")
        st = status.cpu().numpy()                                   # the one synchronisation
    return out, st


def _length(events) -> int:
    if isinstance(events, DeviceEvents):
        return events.num_events
    if isinstance(events, (tuple, list)) and len(events) == 4 and all(torch.is_tensor(e) for e in events):
        return int(events[0].shape[0])
    return len(events)


def _single(events, num_bins, width, height, kind, device):
    if int(num_bins) < 1 or int(width) < 1 or int(height) < 1:          # the reference's asserts (:80-82, :225-227)
        raise ValueError(f"num_bins, width and height must be positive, got {num_bins}, {width}, {height}")
    if isinstance(events, torch.Tensor) and not events.is_cuda:
        raise hip.V2ceHipError(f"events must live on a HIP device (got {events.device}); there is no CPU path")
    grids, st = event_grids_batch(events, [_length(events)], num_bins, height, width, kinds=(kind,), device=device)
    raise_for_status(st, kind)
    return grids


def events_to_voxel_grid(events, num_bins, width, height, device=None) -> torch.Tensor:
    """events_utils.py:70-116: the signed grid, float32 ``[num_bins, height, width]`` on the device.

    Deviation: besides the containers of the other encoders, the reference's ``[N, 4]`` float64 array
    ``[timestamp, x, y, polarity]`` is accepted only if all entries are integral and the polarities are -1, 0 or 1;
    anything else raises ``ValueError``.  The array is left as it was (the reference overwrites its first column)."""
    return _single(events, num_bins, width, height, "signed", device)["signed"][0]


def structured_events_to_voxel_grid(events, num_bins, width, height, device=None) -> torch.Tensor:
    """events_utils.py:215-260: left weights in plane 0, right weights in plane 1, float32 ``[2, num_bins, height,
    width]`` on the device."""
    if isinstance(events, np.ndarray) and events.dtype.names is None:
        raise TypeError("structured_events_to_voxel_grid takes structured events (fields timestamp, x, y, polarity)")
    return _single(events, num_bins, width, height, "split", device)["split"][0]


def structured_events_to_voxel_stat(events, num_bins, width, height, device=None):
    """events_utils.py:333-358: ``(event count, mean, sample std of the in-bin time residue)``, three float64
    ``[2, num_bins, height, width]`` device tensors, plane 1 for polarity 1."""
    if isinstance(events, np.ndarray) and events.dtype.names is None:
        raise TypeError("structured_events_to_voxel_stat takes structured events (fields timestamp, x, y, polarity)")
    g = _single(events, num_bins, width, height, "stat", device)
    return g["stat_count"][0], g["stat_mean"][0], g["stat_std"][0]


# ---------------------------------------------------------------------------------------------------------------------
# command line (v2ce_encode.py)

def build_parser():
    p = argparse.ArgumentParser(description="Encode an events file as voxel grids (events_utils.py), one per frame pair")
    p.add_argument("--events", type=str, required=True,
                   help="events: .npz with key event_stream, or a structured .npy (timestamp, x, y, polarity)")
    p.add_argument("--frame_timestamps", type=str, help="int64 us frame times [N] (.npy): pair i is [T_i, T_i+1)")
    p.add_argument("--fps", type=float, default=None,
                   help="without --frame_timestamps: T_i = int(i * 1 / fps * 1e6); neither: the file is one list")
    p.add_argument("--kind", nargs="+", default=["signed"], choices=list(KINDS))
    p.add_argument("--bins", type=int, default=10)
    p.add_argument("--width", type=int, default=346)
    p.add_argument("--height", type=int, default=260)
    p.add_argument("--chunk", type=int, default=64, help="frame pairs per device call")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("-o", "--out_folder", type=str, default="./results")
    p.add_argument("-l", "--log_level", type=str, default="info")
    return p


def main(argv=None):
    """Writes ``<kind>.npy`` per requested grid (``stat_count.npy``, ``stat_mean.npy``, ``stat_std.npy`` for stat) with
    the pair axis first, and ``status.npy`` (int32 per pair).  A pair without events, or one the stat encoder refuses,
    keeps its zero grids and is reported; bad coordinates or unsorted pairs stop the command."""
    from . import glue
    from .stage2_metrics import load_events, split_by_frames
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()))
    dev = torch.device(args.device)
    if dev.type == "cuda" and dev.index is not None:
        torch.cuda.set_device(dev)
    ev = load_events(args.events)
    if args.frame_timestamps is not None:
        T = np.load(args.frame_timestamps).astype(np.int64).reshape(-1)
    elif args.fps is not None:
        last = int(ev["timestamp"].max()) if len(ev) else 0
        T = [glue.frame_offset_us(0, args.fps)]
        while T[-1] <= last:
            T.append(glue.frame_offset_us(len(T), args.fps))
        T = np.asarray(T, dtype=np.int64)
    else:
        T = None
    if T is None:
        counts, dropped = np.array([len(ev)], np.int64), 0
    else:
        if T.size < 2:
            raise SystemExit("need at least two frame timestamps")
        ev, counts, dropped = split_by_frames(ev, T)
    logger.info(f"{len(ev)} events in {counts.size} lists; {dropped} outside the frame times dropped")
    parts, status = {}, []
    lo = 0
    for c0 in range(0, counts.size, args.chunk):
        c = counts[c0:c0 + args.chunk]
        hi = lo + int(c.sum())
        grids, st = event_grids_batch(ev[lo:hi], c, args.bins, args.height, args.width, kinds=args.kind, device=dev)
        raise_for_status(st & (hip.EVENT_GRIDS_BAD_XY | hip.EVENT_GRIDS_BAD_TIME), f"pairs from {c0}")
        for k, v in grids.items():
            parts.setdefault(k, []).append(v.cpu().numpy())
        status.append(st)
        lo = hi
    status = np.concatenate(status)
    for bit, why in ((hip.EVENT_GRIDS_EMPTY, "have no events"),
                     (hip.EVENT_GRIDS_STAT_TOP_EDGE, "put their last event into bin `bins` (stat grids left zero)"),
                     (hip.EVENT_GRIDS_STAT_OVERFLOW, "overflow the exact sums (stat grids left zero)")):
        if (status & bit).any():
            logger.warning(f"{int((status & bit != 0).sum())} pairs {why}: {np.flatnonzero(status & bit).tolist()[:10]}")
    os.makedirs(args.out_folder, exist_ok=True)
    for k, v in parts.items():
        np.save(op.join(args.out_folder, f"{k}.npy"), np.concatenate(v))
        print(op.join(args.out_folder, f"{k}.npy"))
    np.save(op.join(args.out_folder, "status.npy"), status)


if __name__ == "__main__":
    main()
