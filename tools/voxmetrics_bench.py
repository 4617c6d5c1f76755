"""Rate of the stage-1 score (v2ce_voxmetrics, csrc/voxmetrics.hip) and of the batched voxeliser (v2ce_voxelize_batch,
csrc/voxelize.hip) on one 64-pair 346x260 chunk.

The metric pass reads pred and gt [1, 64, 20, 260, 346] f32 (921 MB) and is timed for pool sizes {2, 4} (the fused
pass alone) and {2, 3, 4} (one generic launch more); GB/s counts those 921 MB.  The voxeliser takes about 190 k events
per pair (LDATI output of synthetic voxels) and is compared with a loop of single-list calls of
v2ce_voxelize_events.  HIP events, median of --iters after --warmup; prints one JSON line (--out writes it)."""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, P = 260, 346, a.pairs
    L = hip.lib()
    st = hip.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand((1, P, 20, H, W), device="cuda", generator=g) * 0.03
    gt = torch.rand((1, P, 20, H, W), device="cuda", generator=g) * 0.03
    nbytes = 2 * pred.numel() * 4
    rec = {"tool": "tools/voxmetrics_bench.py", "device": torch.cuda.get_device_name(0), "pairs": P, "H": H, "W": W,
           "metric_bytes": nbytes}
    for name, ks in (("k24", (2, 4)), ("k234", (2, 3, 4))):
        karr = (ctypes.c_int * len(ks))(*ks)
        nb = L.v2ce_voxmetrics_workspace_bytes(1, P, 20, H, W, karr, len(ks))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        out = torch.empty(ctypes.sizeof(hip.VoxMetricsStats), dtype=torch.uint8, device="cuda")

        def call():
            hip.check(L.v2ce_voxmetrics(pred.data_ptr(), gt.data_ptr(), 1, P, 20, H, W, 0.01, karr, len(ks),
                                        out.data_ptr(), ctypes.sizeof(hip.VoxMetricsStats), ws.data_ptr(), nb, st),
                      "v2ce_voxmetrics")
        med, mn = timed(call, a.warmup, a.iters)
        rec[f"metric_{name}_ms"] = round(med, 4)
        rec[f"metric_{name}_ms_min"] = round(mn, 4)
        rec[f"metric_{name}_GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)
    del pred, gt
    torch.cuda.empty_cache()
    vox = torch.from_numpy(synth.synthetic_voxels(P, H, W, seed=5, regime="sparse") * np.float32(0.3)).cuda()
    ev = ldati_device(vox, fps=30, seed=1)
    ts, x, y, p = ev._unpacked()
    counts = np.asarray(ev.frame_counts, np.int64)
    n = int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    offd = torch.from_numpy(off).cuda()
    nb = L.v2ce_voxelize_batch_workspace_bytes(P, 10, H, W, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    vol = torch.empty((P, 20, H, W), device="cuda")
    status = torch.empty(P, dtype=torch.int32, device="cuda")

    def vb():
        hip.check(L.v2ce_voxelize_batch(ts.data_ptr(), x.data_ptr(), y.data_ptr(), p.data_ptr(), offd.data_ptr(), n, P,
                                        10, H, W, None, vol.data_ptr(), status.data_ptr(), ws.data_ptr(), nb, st),
                  "v2ce_voxelize_batch")
    med, mn = timed(vb, a.warmup, a.iters)
    rng = torch.empty(2, dtype=torch.int64, device="cuda")
    one = torch.empty((20, H, W), device="cuda")

    def loop():   # the existing single-list voxeliser, one call and one range read per pair (what the drop-in does)
        for i in range(P):
            lo = int(off[i])
            hip.check(L.v2ce_voxelize_events(ts[lo:].data_ptr(), x[lo:].data_ptr(), y[lo:].data_ptr(), p[lo:].data_ptr(),
                                             int(counts[i]), 10, H, W, one.data_ptr(), rng.data_ptr(), st),
                      "v2ce_voxelize_events")
            rng.cpu()
    lmed, _ = timed(loop, 1, max(3, a.iters // 4))
    rec.update({"voxelize_events": n, "voxelize_events_per_pair": round(n / P), "voxelize_batch_ms": round(med, 4),
                "voxelize_batch_ms_min": round(mn, 4), "voxelize_loop_ms": round(lmed, 4),
                "voxelize_status_nonzero": int((status != 0).sum().item()), "iters": a.iters, "warmup": a.warmup,
                "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
