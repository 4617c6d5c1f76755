"""Time of the event -> grid encoders (v2ce_event_grids_batch, csrc/voxelize.hip) on 64 full-size lists: the LDATI
events of synthetic `stress` voxels at 346x260, encoded as signed + split + stat grids in one call, and each kind alone,
against the NumPy restatement of the reference (np.add.at, as events_utils.py:70-116, :215-260, :333-358 do it) on the
same events on the host.  HIP events for the device (median of --iters after --warmup), wall clock for NumPy (--numpy_pairs
lists, scaled to all).  Prints one JSON line (--out writes it).  A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from v2ce_toolbox_amd import hip, synth  # noqa: E402
from v2ce_toolbox_amd.LDATI import ldati_device  # noqa: E402


def timed(call, warmup, iters):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def numpy_grids(t, x, y, p, bins, W, H):
    """The reference's three encoders on one list (host arrays), without writing to the inputs."""
    first, last = t[0], t[-1]
    dT = last - first
    dT = 1.0 if dT == 0 else dT
    ts = (bins - 1) * (t - first) / dT
    xs, ys = x.astype(int), y.astype(int)
    pols = np.where(p == 0, -1, p)
    tis = ts.astype(int)
    dts = ts - tis
    left, right = pols * (1.0 - dts), pols * dts
    signed = np.zeros(bins * H * W, np.float32)
    split = np.zeros((2, bins * H * W), np.float32)
    v = tis < bins
    il = xs[v] + ys[v] * W + tis[v] * W * H
    np.add.at(signed, il, left[v])
    np.add.at(split[0], il, left[v])
    v = (tis + 1) < bins
    ir = xs[v] + ys[v] * W + (tis[v] + 1) * W * H
    np.add.at(signed, ir, right[v])
    np.add.at(split[1], ir, right[v])
    delta_t = int(np.ceil((last - first) / bins))
    d = t - first
    with np.errstate(divide="ignore"):
        tbs, trs = d // delta_t, d % delta_t
    ps = np.where(p == 1, 1, 0)
    keep = tbs < bins                                   # the reference raises here; the device flags the list
    idx = (ps[keep], tbs[keep], ys[keep], xs[keep])
    cnt, s, ss = (np.zeros((2, bins, H, W)) for _ in range(3))
    np.add.at(cnt, idx, 1)
    np.add.at(s, idx, trs[keep])
    np.add.at(ss, idx, trs[keep] ** 2)
    mean = s / np.maximum(cnt, 1)
    with np.errstate(invalid="ignore"):
        std = np.sqrt((ss - (s ** 2) / np.maximum(cnt, 1)) / np.maximum(cnt - 1, 1))
    return signed, split, cnt, mean, std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--numpy_pairs", type=int, default=4)
    ap.add_argument("--commit", type=str, default=None, help="recorded as given (the GPU box may have no .git)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, P, bins = 260, 346, a.pairs, a.bins
    L = hip.lib()
    st = hip.stream_ptr()
    vox = torch.from_numpy(synth.synthetic_voxels(P, H, W, seed=5, regime="stress")).cuda()
    ev = ldati_device(vox, fps=30, seed=1)
    ts, x, y, p = ev._unpacked()
    del vox
    counts = np.asarray(ev.frame_counts, np.int64)
    n = int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    offd = torch.from_numpy(off).cuda()
    nb = L.v2ce_event_grids_workspace_bytes(P, bins, H, W, n, 7)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    signed = torch.empty((P, bins, H, W), device="cuda")
    split = torch.empty((P, 2, bins, H, W), device="cuda")
    cnt, mean, std = (torch.empty((P, 2, bins, H, W), dtype=torch.float64, device="cuda") for _ in range(3))
    status = torch.empty(P, dtype=torch.int32, device="cuda")
    rec = {"tool": "tools/event_grids_bench.py", "device": torch.cuda.get_device_name(0), "pairs": P, "H": H, "W": W,
           "bins": bins, "events": n, "events_per_pair": round(n / P), "commit": a.commit}
    for name, kinds in (("all", 7), ("signed", 1), ("split", 2), ("stat", 4)):
        def call():
            hip.check(L.v2ce_event_grids_batch(ts.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), offd.data_ptr(),
                                               n, P, bins, H, W, kinds, signed.data_ptr(), split.data_ptr(),
                                               cnt.data_ptr(), mean.data_ptr(), std.data_ptr(), status.data_ptr(),
                                               ws.data_ptr(), nb, st), "v2ce_event_grids_batch")
        med, mn = timed(call, a.warmup, a.iters)
        rec[f"device_{name}_ms"] = round(med, 4)
        rec[f"device_{name}_ms_min"] = round(mn, 4)
        rec[f"device_{name}_Mevents_per_s"] = round(n / (med * 1e-3) / 1e6, 1)
        rec[f"status_nonzero_{name}"] = int((status != 0).sum().item())
    host = [c.cpu().numpy() for c in (ts, x, y, p)]
    k = max(1, min(a.numpy_pairs, P))
    t0 = time.perf_counter()
    for i in range(k):
        lo, hi = int(off[i]), int(off[i + 1])
        numpy_grids(*(c[lo:hi] for c in host), bins, W, H)
    dt = time.perf_counter() - t0
    nk = int(off[k])
    rec.update({"numpy_pairs_timed": k, "numpy_ms_timed": round(dt * 1e3, 1),
                "numpy_all_ms_scaled_to_all_pairs": round(dt * 1e3 * n / max(nk, 1), 1),
                "speedup_all_kinds": round(dt * 1e3 * n / max(nk, 1) / rec["device_all_ms"], 1),
                "iters": a.iters, "warmup": a.warmup, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
