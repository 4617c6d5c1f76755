"""Independent NumPy restatement of events_to_voxel_grid, structured_events_to_voxel_grid and
structured_events_to_voxel_stat (train/scripts/utils/events_utils.py:70-116, :215-260, :333-358) with explicit per-cell
loops instead of np.add.at, and the rounding of every accumulation spelled out.

A cell of the float grids receives, in this order, the LEFT weights of the events whose truncated normalised time is
its bin (first np.add.at call), then the RIGHT weights of the events of the bin before (second call), each group in
event order.  The grids are float32 and the weights float64, and np.add.at adds them as

    acc = float32(float64(acc) + v)            (``exact_add``)

not as float32(acc + float32(v)) (``f32_add``, kept here only so that a test can show the fixtures tell them apart).

The statistics are integer sums (count, sum of residues, sum of squared residues) per (polarity plane, bin, pixel);
the reference accumulates them in float64, which is exact below 2^53, and finalises them in float64.  Inputs are never
modified.  Not collected by pytest."""
import numpy as np

EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])


def exact_add(acc, v):
    return np.float32(np.float64(acc) + np.float64(v))


def f32_add(acc, v):
    return np.float32(np.float32(acc) + np.float32(v))


def _weights(events, bins):
    """Per event: (tis, left weight, right weight) as Python int / float64 (:87-104, :232-248)."""
    t = np.asarray(events["timestamp"], dtype=np.int64)
    first, last = int(t[0]), int(t[-1])                       # IndexError on an empty list, like events[-1]
    delta = np.float64(last - first) if last != first else np.float64(1.0)
    ts = (np.float64(bins - 1) * (t - first).astype(np.float64)) / delta
    tis = ts.astype(np.int64)
    dts = ts - tis.astype(np.float64)
    pol = np.asarray(events["polarity"]).astype(np.float64)
    pol = np.where(pol == 0, -1.0, pol)
    return tis, pol * (1.0 - dts), pol * dts


def _check(events, H, W):
    t = np.asarray(events["timestamp"], dtype=np.int64)
    if ((events["x"] < 0) | (events["x"] >= W) | (events["y"] < 0) | (events["y"] >= H)).any():
        raise ValueError("coordinates outside the grid")
    if ((t < t[0]) | (t > t[-1])).any():
        raise ValueError("timestamp outside [first, last]")


def _cells(events, bins, W):
    """cell (bin, y, x) -> ([lefts in event order], [rights in event order])."""
    tis, left, right = _weights(events, bins)
    cells = {}
    for i in range(len(tis)):
        b, y, x = int(tis[i]), int(events["y"][i]), int(events["x"][i])
        if b < bins:
            cells.setdefault((b, y, x), ([], []))[0].append(left[i])
        if b + 1 < bins:
            cells.setdefault((b + 1, y, x), ([], []))[1].append(right[i])
    return cells


def events_to_voxel_grid(events, bins, W, H, add=exact_add):
    """:70-116 on structured events: float32 [bins, H, W]."""
    _check(events, H, W)
    grid = np.zeros((bins, H, W), np.float32)
    for cell, (lefts, rights) in _cells(events, bins, W).items():
        acc = np.float32(0)
        for v in lefts:
            acc = add(acc, v)
        for v in rights:
            acc = add(acc, v)
        grid[cell] = acc
    return grid


def structured_events_to_voxel_grid(events, bins, W, H, add=exact_add):
    """:215-260: float32 [2, bins, H, W], lefts in plane 0, rights in plane 1."""
    _check(events, H, W)
    grid = np.zeros((2, bins, H, W), np.float32)
    for cell, groups in _cells(events, bins, W).items():
        for plane, vals in enumerate(groups):
            acc = np.float32(0)
            for v in vals:
                acc = add(acc, v)
            grid[(plane,) + cell] = acc
    return grid


def structured_events_to_voxel_stat(events, bins, W, H):
    """:333-358: (count, mean, std), float64 [2, bins, H, W]."""
    _check(events, H, W)
    t = np.asarray(events["timestamp"], dtype=np.int64)
    first, last = int(t[0]), int(t[-1])
    delta_t = int(np.ceil(np.float64(last - first) / np.float64(bins)))
    cells = {}
    for i in range(len(t)):
        d = int(t[i]) - first
        tb, tr = (d // delta_t, d % delta_t) if delta_t else (0, 0)      # NumPy: integer // 0 and % 0 give 0
        if tb >= bins:
            raise IndexError(f"index {tb} is out of bounds for axis 1 with size {bins}")
        key = (1 if int(events["polarity"][i]) == 1 else 0, tb, int(events["y"][i]), int(events["x"][i]))
        n, s, ss = cells.get(key, (0, 0, 0))
        cells[key] = (n + 1, s + tr, ss + tr * tr)
    count, mean, std = (np.zeros((2, bins, H, W), np.float64) for _ in range(3))
    with np.errstate(invalid="ignore"):
        for key, (n, s, ss) in cells.items():
            if ss >= 2 ** 53:
                raise ValueError("sum of squared residues reached 2^53")
            N, S, SS = np.float64(n), np.float64(s), np.float64(ss)
            d1, d2 = max(N, np.float64(1)), max(N - np.float64(1), np.float64(1))
            var = (SS - (S * S) / d1) / d2
            count[key], mean[key], std[key] = N, S / d1, np.sqrt(var)
    return count, mean, std


# the fixtures of tests/make_event_grids_goldens.py (tests/golden/.evgrids/<name>.npz)
GOLDEN_NAMES = ("cell40_b5", "cell5000_b16", "trap_b5", "random_b1", "random_b16", "one_event_b5", "same_stamp_b5",
                "on_last_stamp_b5", "pol_0_m1_mixed_b5", "span_not_multiple_b10", "stat_777_b10", "six_residues_b10",
                "big_residues_b2", "top_edge_b10", "negative_var_b2")
STAT_KEYS = ("stat_count", "stat_mean", "stat_std")
