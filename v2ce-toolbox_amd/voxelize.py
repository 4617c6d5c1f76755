"""Events -> discretised event volume on the device (the inverse of LDATI).

Drop-in for ``gen_discretized_event_volume(events, vol_size)`` of
``train/scripts/utils/events_utils.py:147-175`` (the authors' round-trip sanity check,
``train/scripts/stage2/stage2_metrics.py:187-190``): same argument meaning, the volume comes back as
a float32 torch tensor ``[2*bins, H, W]`` -- on the device here.  There is no CPU path.  Polarity 0 and -1 both go
to the negative half (events_utils.py:153 maps 0 to -1, :133-136 send p < 0 there).

``gen_discretized_event_volume_batch`` voxelises many event lists (frame pairs) in one call through
``v2ce_voxelize_batch``: each cell is summed in the order of the reference's serial ``put_``, so the volumes are
bit-identical to the reference's on one thread and to each other run to run.
"""
from __future__ import annotations

from typing import Sequence, Union

import numpy as np
import torch

from . import hip
from .LDATI import EVENT_DTYPE, DeviceEvents


def _soa(events, device):
    if isinstance(events, DeviceEvents):
        return events.ts, events.x, events.y, events.p
    if isinstance(events, (tuple, list)) and len(events) == 4 and all(torch.is_tensor(e) for e in events):
        return tuple(events)
    ev = np.asarray(events)
    if ev.dtype.names is None or not {"timestamp", "x", "y", "polarity"} <= set(ev.dtype.names):
        raise TypeError("events must be a structured array with fields timestamp, x, y, polarity "
                        "(the LDATI record dtype), a DeviceEvents or a (ts, x, y, p) tuple of device tensors")
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt, copy=False))).to(device)
    return (to(ev["timestamp"], np.int64), to(ev["x"], np.int16), to(ev["y"], np.int16), to(ev["polarity"], np.int8))


def gen_discretized_event_volume(events: Union[np.ndarray, DeviceEvents, Sequence[torch.Tensor]], vol_size,
                                 device="cuda") -> torch.Tensor:
    """events_utils.py:147-175.  ``vol_size = (2*bins, H, W)``."""
    nb2, H, W = (int(v) for v in vol_size)
    if nb2 < 4 or nb2 % 2:
        raise ValueError(f"vol_size[0] must be an even number >= 4, got {nb2}")
    if not isinstance(events, (DeviceEvents, tuple, list)) and len(events) == 0:
        raise RuntimeError("gen_discretized_event_volume: no events (the reference raises on t.min() of an empty tensor)")
    ts, x, y, p = _soa(events, device)
    for t, dt, name in ((ts, torch.int64, "timestamp"), (x, torch.int16, "x"), (y, torch.int16, "y"), (p, torch.int8, "polarity")):
        if not t.is_cuda:
            raise hip.V2ceHipError(f"{name} must live on a HIP device; there is no CPU path")
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} tensor")
    n = int(ts.shape[0])
    if n == 0:
        raise RuntimeError("gen_discretized_event_volume: no events (the reference raises on t.min() of an empty tensor)")
    # events_utils.py:129-130 assert the coordinates: checked on the device, fetched together with the
    # time range in ONE small D2H copy after the launch
    bad = ((x < 0) | (x >= W) | (y < 0) | (y >= H)).any().to(torch.int64).reshape(1)
    vol = torch.empty((nb2, H, W), dtype=torch.float32, device=ts.device)
    rng = torch.empty(2, dtype=torch.int64, device=ts.device)
    with torch.cuda.device(ts.device):
        hip.check(hip.lib().v2ce_voxelize_events(ts.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), n, nb2 // 2,
                                                 H, W, vol.data_ptr(), rng.data_ptr(), hip.stream_ptr(ts.device)),
                  "v2ce_voxelize_events")
    t_min, t_max, is_bad = (int(v) for v in torch.cat([rng, bad]).tolist())
    if is_bad:
        raise AssertionError("gen_discretized_event_volume: event coordinates outside the volume")
    if t_max == t_min:
        raise RuntimeError("gen_discretized_event_volume: t_max == t_min (the reference divides by zero here)")
    return vol


def gen_discretized_event_volume_batch(events, counts, bins: int, H: int, W: int, t_range=None,
                                       device=None):
    """P event lists -> ``(volume [P, 2*bins, H, W] f32 device tensor, status int32 [P] numpy)``.

    ``events``: host structured array (fields timestamp, x, y, polarity), or a (ts, x, y, p) tuple of device tensors,
    with the lists back to back; ``counts`` [P] the length of each.  Each pair is rescaled over its own [t_min, t_max]
    or over ``t_range[i] = (t_min, t_max)`` (the t_min / t_max of gen_discretized_event_volume_from_tensor,
    events_utils.py:177-211).  ``bins`` in [2, 16].  status bits (hip.VOXELIZE_*): 1 empty pair, 2 a single timestamp
    (the reference divides by zero): both get a zero volume.  Coordinates outside H x W raise AssertionError (the
    reference's assert); an explicit range with t_max < t_min raises ValueError.  One host synchronisation."""
    bins, H, W = int(bins), int(H), int(W)
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    P = c.size
    if P == 0:
        raise ValueError("no pairs")
    if (c < 0).any():
        raise ValueError("negative count")
    if not 2 <= bins <= 16:
        raise ValueError(f"bins must lie in [2, 16], got {bins}")
    if isinstance(events, np.ndarray):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if events.dtype.names is None or not {"timestamp", "x", "y", "polarity"} <= set(events.dtype.names):
            raise TypeError("events must have the fields timestamp, x, y, polarity")
        cols = [np.array(events[f], dtype=dt) for f, dt in
                (("timestamp", np.int64), ("x", np.int16), ("y", np.int16), ("polarity", np.int8))]
        if torch.device(dev).type != "cuda":
            raise hip.V2ceHipError(f"device {dev} is not a HIP device; there is no CPU path")
        ts, x, y, p = (torch.from_numpy(a).to(dev) for a in cols)
    else:
        ts, x, y, p = _soa(events, device)
        for t, dt, name in ((ts, torch.int64, "timestamp"), (x, torch.int16, "x"), (y, torch.int16, "y"),
                            (p, torch.int8, "polarity")):
            if not t.is_cuda:
                raise hip.V2ceHipError(f"{name} must live on a HIP device; there is no CPU path")
            if t.dtype != dt or not t.is_contiguous():
                raise TypeError(f"{name} must be a contiguous {dt} tensor")
        dev = ts.device
    n = int(ts.shape[0])
    if int(c.sum()) != n:
        raise ValueError(f"counts add up to {int(c.sum())}, the events are {n}")
    L = hip.lib()
    ws_bytes = L.v2ce_voxelize_batch_workspace_bytes(P, bins, H, W, n)
    if ws_bytes == 0:
        raise hip.V2ceHipError(f"v2ce_voxelize_batch: unsupported shape P={P}, bins={bins}, H={H}, W={W}, n={n}")
    with torch.cuda.device(dev):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        rng = None
        if t_range is not None:
            r = np.asarray(t_range, dtype=np.int64).reshape(P, 2)
            rng = torch.from_numpy(np.ascontiguousarray(r)).to(dev)
        vol = torch.empty((P, 2 * bins, H, W), dtype=torch.float32, device=dev)
        status = torch.empty(P, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if n else None
        hip.check(L.v2ce_voxelize_batch(ptr(ts), ptr(x), ptr(y), ptr(p), off.data_ptr(), n, P, bins, H, W,
                                        None if rng is None else rng.data_ptr(), vol.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), ws_bytes, hip.stream_ptr(dev)), "v2ce_voxelize_batch")
        st = status.cpu().numpy()                                   # the one synchronisation
    if (st & hip.VOXELIZE_BAD_XY).any():
        raise AssertionError(f"gen_discretized_event_volume_batch: event coordinates outside the volume in pairs "
                             f"{np.flatnonzero(st & hip.VOXELIZE_BAD_XY).tolist()[:10]}")
    if (st & hip.VOXELIZE_BAD_RANGE).any():
        raise ValueError(f"t_range with t_max < t_min in pairs {np.flatnonzero(st & hip.VOXELIZE_BAD_RANGE).tolist()[:10]}")
    return vol, st
