"""Times of the device event-frame video (csrc/event_frames.hip, event_frames.EventFrameRenderer) on one GPU.

End of clip: ``finish()`` (two refinement passes, render, one download of the uint8 frames) against the host path on the
same sums (torch.cat + .cpu() + v2ce.event_frame_images), --pairs frame pairs at 260x346 in batches of 64, both modes,
alternating, --reps repetitions each; host clock around a device synchronise; the frames of both are compared.
Per batch: the fused kernel (v2ce_event_frames_sums) against pipeline.event_frame_sums on [64,2,10,260,346], HIP events,
median of --iters; GB/s counts 92 B per pixel-pair (80 read, 12 written).  Prints one JSON line (--out writes it)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from v2ce_toolbox_amd import hip, pipeline  # noqa: E402
from v2ce_toolbox_amd import v2ce as cli  # noqa: E402
from v2ce_toolbox_amd.event_frames import EventFrameRenderer  # noqa: E402

H, W, B = 260, 346, 64


def batch(i, n):
    g = torch.Generator(device="cuda").manual_seed(100 + i)
    return torch.relu(0.8 * torch.randn((n, 2, 10, H, W), device="cuda", generator=g))


def fill(r, pairs):
    for i, a in enumerate(range(0, pairs, B)):
        r.add(a, batch(i, min(B, pairs - a)))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2047)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    rec = {"tool": "tools/event_frames_bench.py", "device": torch.cuda.get_device_name(0), "pairs": a.pairs, "H": H, "W": W,
           "batch": B, "reps": a.reps}
    warm = EventFrameRenderer(True, 10, 98, H, W, "cuda")
    fill(warm, B)
    warm.finish()
    for keep, name in ((True, "polarity"), (False, "grey")):
        dev_s, host_s, same = [], [], True
        for _ in range(a.reps):
            r = EventFrameRenderer(keep, 10, 98, H, W, "cuda")
            fill(r, a.pairs)
            sums = list(r._sums)
            t0 = time.perf_counter()
            frames, upper = r.finish()
            torch.cuda.synchronize()
            dev_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ef = torch.cat([t for _, t in sorted(sums, key=lambda kv: kv[0])]).cpu().numpy()
            want = cli.event_frame_images(ef, 10, 98, keep)
            host_s.append(time.perf_counter() - t0)
            same = same and frames.tobytes() == want.tobytes()
            del sums, ef, want, frames, r
            torch.cuda.empty_cache()
        rec[name] = {"device_finish_s": [round(t, 4) for t in dev_s], "host_path_s": [round(t, 4) for t in host_s],
                     "ratio_host_over_device": [round(h / d, 1) for h, d in zip(host_s, dev_s)], "frames_equal": bool(same),
                     "device_faster_in_every_repetition": all(d < h for d, h in zip(dev_s, host_s))}
    vox = batch(0, B)
    r = EventFrameRenderer(True, 10, 98, H, W, "cuda")

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def fused():
        r._sums = []
        r.add(0, vox)
    nbytes = 92 * B * H * W
    f_ms, t_ms = timed(fused), timed(lambda: pipeline.event_frame_sums(vox))
    rec["per_batch"] = {"fused_ms": round(f_ms, 4), "torch_event_frame_sums_ms": round(t_ms, 4), "bytes": nbytes,
                        "fused_GBps": round(nbytes / (f_ms * 1e-3) / 1e9, 1), "iters": a.iters}
    rec.update({"time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
