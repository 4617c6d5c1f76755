"""Time of the physical-attention maps (v2ce_physatt_batch, csrc/physatt.hip) on 64 full-size pairs: a 65-frame clip at
346x260 with about 20 000 uniformly placed events per pair, pool 8, ceiling 25 (the call of the reference's
tools/gen_phy_att.py), each mode alone, and the log-frame residual of the same clip; against the same arithmetic in NumPy
on the host with a Python loop over the events, as physical_att.py:41-44 has it (--numpy_pairs pairs, scaled to all).
HIP events for the device (median over --iters windows of --reps calls, after --warmup), wall clock for NumPy.  The
record states the bytes each call must move next to its time.  Prints one JSON line (--out writes it).  A record, not a
gate."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from v2ce_toolbox_amd import hip  # noqa: E402
from v2ce_toolbox_amd import physical_att as PA  # noqa: E402


def timed(call, warmup, iters, reps):
    """ms per call: `iters` windows of `reps` back-to-back calls between two HIP events; (median, min) over the windows."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ms)), float(np.min(ms))


def numpy_pair(x, y, frames, pool, ceiling, lut, w):
    """physical_attention_generation_advanced on one pair (host arrays), the event loop as the reference has it."""
    H, W = frames.shape[1:]
    cnt = np.zeros((H, W), dtype="int")
    for ex, ey in zip(x.tolist(), y.tolist()):
        cnt[ey, ex] += 1
    Hp, Wp = -(-H // pool), -(-W // pool)

    def mosaic(img):
        pad = np.zeros((Hp * pool, Wp * pool), np.float32)
        pad[:H, :W] = img
        return pad.reshape(Hp, pool, Wp, pool).transpose(0, 2, 1, 3).mean(axis=(2, 3))

    ev = mosaic(cnt)
    ev[ev < 0.05] = 0
    r = np.clip(ev / (mosaic(np.abs(lut[frames[1]] - lut[frames[0]])) + 1e-3), 0, 2 * ceiling)
    for axis in (0, 1):
        a = np.moveaxis(r, axis, 0).astype(np.float64)
        idx = np.arange(-4, a.shape[0] + 4) % (2 * a.shape[0])
        a = a[np.where(idx < a.shape[0], idx, 2 * a.shape[0] - 1 - idx)]
        n = a.shape[0] - 8
        out = a[4:4 + n] * w[0]
        for j in range(4, 0, -1):
            out = out + (a[4 - j:4 - j + n] + a[4 + j:4 + j + n]) * w[j]
        r = np.moveaxis(out.astype(np.float32), 0, axis)
    r = np.clip(r, 0, ceiling)
    return (r - r.min()) / (r.max() - r.min()) if r.max() != r.min() else np.zeros_like(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--events_per_pair", type=int, default=20000)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--ceiling", type=float, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--numpy_pairs", type=int, default=2)
    ap.add_argument("--commit", type=str, default=None, help="recorded as given (the GPU box may have no .git)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, P, pool = 260, 346, a.pairs, a.pool
    Hp, Wp = -(-H // pool), -(-W // pool)
    rng = np.random.default_rng(5)
    clip = rng.integers(0, 256, (P + 1, H, W)).astype(np.uint8)
    clip[1:] = np.clip(clip[:-1].astype(int) + rng.integers(-9, 10, (P, H, W)), 0, 255)
    counts = rng.integers(a.events_per_pair * 3 // 4, a.events_per_pair * 5 // 4, P).astype(np.int64)
    n = int(counts.sum())
    xh, yh = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    L = hip.lib()
    st = hip.stream_ptr()
    fr, x, y, offd = (torch.from_numpy(v).cuda() for v in (clip, xh, yh, off))
    nb = L.v2ce_physatt_workspace_bytes(P, H, W, pool, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    maps = torch.empty((P, Hp, Wp), device="cuda")
    masks = torch.empty((P, Hp, Wp), dtype=torch.uint8, device="cuda")
    status = torch.empty(P, dtype=torch.int32, device="cuda")
    lfr = torch.empty((P, 1, H, W), device="cuda")
    lut_att, lut_plain = PA._lut(1e-6, fr.device), PA._lut(0.0, fr.device)
    gw = PA.gauss_weights()
    gwp = gw.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    in_bytes = 2 * P * H * W + 4 * n                    # two u8 frames per pair as the kernels read them + x, y int16
    rec = {"tool": "tools/physatt_bench.py", "device": torch.cuda.get_device_name(0), "pairs": P, "H": H, "W": W,
           "pool": pool, "ceiling": a.ceiling, "events": n, "events_per_pair": round(n / P), "commit": a.commit,
           "physatt_bytes_in": in_bytes, "physatt_bytes_out": 4 * P * Hp * Wp,
           "lfr_bytes_in": (P + 1) * H * W, "lfr_bytes_out": 4 * P * H * W}
    for name, mode, K in (("advanced", hip.PHYSATT_ADVANCED, 0), ("plain", hip.PHYSATT_PLAIN, 0),
                          ("ratio_mask", hip.PHYSATT_RATIO, 16)):
        def call():
            hip.check(L.v2ce_physatt_batch(fr.data_ptr(), 1, P, H, W, x.data_ptr(), y.data_ptr(), offd.data_ptr(), n, pool,
                                           mode, a.ceiling, 0.6, K, lut_att.data_ptr(), gwp, maps.data_ptr(),
                                           masks.data_ptr(), status.data_ptr(), ws.data_ptr(), nb, st), "v2ce_physatt_batch")
        med, mn = timed(call, a.warmup, a.iters, a.reps)
        rec[f"device_{name}_ms"] = round(med, 4)
        rec[f"device_{name}_ms_min"] = round(mn, 4)
        rec[f"device_{name}_GBps_in"] = round(in_bytes / (med * 1e-3) / 1e9, 1)
        rec[f"status_nonzero_{name}"] = int((status != 0).sum().item())

    def residual():
        hip.check(L.v2ce_log_residual_batch(fr.data_ptr(), P + 1, H, W, lut_plain.data_ptr(), lfr.data_ptr(), st),
                  "v2ce_log_residual_batch")
    med, mn = timed(residual, a.warmup, a.iters, a.reps)
    rec.update({"device_lfr_ms": round(med, 4), "device_lfr_ms_min": round(mn, 4),
                "device_lfr_GBps": round((rec["lfr_bytes_in"] + rec["lfr_bytes_out"]) / (med * 1e-3) / 1e9, 1)})
    k = max(1, min(a.numpy_pairs, P))
    lut_h = PA.lin_log_lut(1e-6)
    t0 = time.perf_counter()
    for i in range(k):
        numpy_pair(xh[off[i]:off[i + 1]], yh[off[i]:off[i + 1]], clip[i:i + 2], pool, a.ceiling, lut_h, gw)
    dt = time.perf_counter() - t0
    rec.update({"numpy_pairs_timed": k, "numpy_ms_timed": round(dt * 1e3, 1),
                "numpy_ms_scaled_to_all_pairs": round(dt * 1e3 * P / k, 1),
                "speedup_advanced": round(dt * 1e3 * P / k / rec["device_advanced_ms"], 1),
                "iters": a.iters, "reps": a.reps, "warmup": a.warmup, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
