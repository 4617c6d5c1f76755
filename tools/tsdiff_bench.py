"""Rate of the stage-2 score kernel (v2ce_tsdiff, csrc/tsdiff.hip) on one 64-pair chunk at bench density.

The predicted events are LDATI output of the synthetic-weight model at 346x260; a second LDATI draw with another
seed stands in for the recording.  Times r = 0, 1, 2 with HIP events (median of --iters calls after --warmup) and
prints one JSON line per r plus a summary line; --out writes the record (profiles/)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from v2ce_toolbox_amd import glue, hip, synth  # noqa: E402
from v2ce_toolbox_amd.LDATI import ldati_device  # noqa: E402
from v2ce_toolbox_amd.v2ce_3d import V2ce3d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, P = 260, 346, a.pairs
    model = V2ce3d()
    model.load_state_dict(synth.make_state_dict(0))
    model = model.eval().cuda()
    vox = glue.video_to_voxels(model, synth.synthetic_frames(P + 1, H, W), width=W, height=H, device="cuda")
    pred = ldati_device(vox, fps=30, seed=1)
    gt = ldati_device(vox, fps=30, seed=2)
    p, g = pred._unpacked(), gt._unpacked()
    pc, gc = pred.frame_counts, gt.frame_counts
    poff = np.concatenate([[0], np.cumsum(pc)]).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum(gc)]).astype(np.int64)
    offs = torch.from_numpy(np.concatenate([goff, poff])).cuda()
    fps = torch.full((P,), 30.0, dtype=torch.float64, device="cuda")
    L = hip.lib()
    nb = L.v2ce_tsdiff_workspace_bytes(P, H, W, int(poff[-1]))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    stats = torch.empty(3 * P, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = hip.stream_ptr()
    recs = []
    for r in (0, 1, 2):
        def call():
            hip.check(L.v2ce_tsdiff(*(t.data_ptr() for t in g), offs.data_ptr(), int(goff[-1]), *(t.data_ptr() for t in p),
                                    offs[P + 1:].data_ptr(), int(poff[-1]), fps.data_ptr(), P, H, W, r, None,
                                    stats.data_ptr(), status.data_ptr(), ws.data_ptr(), nb, st), "v2ce_tsdiff")
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert int(status.item()) == 0
        s = stats.cpu().numpy().reshape(P, 3)
        med = float(np.median(ms))
        rec = {"r": r, "pairs": P, "gt_events": int(goff[-1]), "pred_events": int(poff[-1]), "ms_per_chunk": round(med, 4),
               "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4),
               "gt_events_per_s": round(goff[-1] / (med * 1e-3)), "overflow": int(s[:, 1].sum()),
               "avg_error": float(((s[:, 0] + s[:, 1] * (1e6 / 30 / 10 * 3)) / s[:, 2]).mean())}
        print(json.dumps(rec))
        recs.append(rec)
    out = {"tool": "tools/tsdiff_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "warmup": a.warmup, "workspace_bytes": int(nb), "target_ms_r0": 2.0, "records": recs,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), **hip.provenance()}
    print(json.dumps({"summary": {f"r{x['r']}_ms": x["ms_per_chunk"] for x in recs}}))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
