"""Rate of the stage-1 loss pass (v2ce_voxlosses, csrc/voxlosses.hip) on 64 pairs of 346x260 as [4, 16, 20, 260, 346].

One call reads pred and gt (2 x 4 bytes x numel = 921 MB) and writes the statistics of every term.  It is timed with
all terms, with match left out (the term that costs an f64 exp per value) and with the elementwise sums alone, per
``synth.synthetic_voxels`` regime.  "fraction_of_stream" is the algorithmic bytes over the time, as a fraction of the
6.3 TB/s that streaming reads reach on the MI355X: a whole-call figure, not a kernel's share of peak.  The comparison
computes the same terms with plain torch device ops (written for this tool; f32, as the reference runs them) and is
checked against the statistics before it is timed.  HIP events around each call, median of --iters after --warmup;
prints one JSON line (--out writes it)."""
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
from v2ce_toolbox_amd import losses as VL  # noqa: E402

STREAM_BPS = 6.3e12


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


def torch_terms(p, g):
    """The default terms plus pt, match and the norms with torch device ops: what a user would write today."""
    F = torch.nn.functional
    B, L, C, H, W = p.shape
    vol = lambda t: t.reshape(B, L, 2, 10, H, W).permute(0, 2, 1, 3, 4, 5).reshape(B * 2, L * 10, H, W)
    pv, gv = vol(p), vol(g)
    out = {"mse": F.mse_loss(p, g)}
    out["pyramid"] = sum(F.mse_loss(F.avg_pool3d(pv, k, k), F.avg_pool3d(gv, k, k)) for k in (2, 4, 8)) / 3
    pt, gt_ = (t.reshape(B * 2, L * 10, H * W).transpose(1, 2) for t in (pv, gv))
    out["pt"] = (F.mse_loss(pt, gt_) + F.mse_loss(F.avg_pool1d(pt, 3, 3, 1), F.avg_pool1d(gt_, 3, 3, 1)) +
                 F.mse_loss(F.avg_pool1d(pt, 5, 5), F.avg_pool1d(gt_, 5, 5))) / 2
    ap, ag = p.abs(), g.abs()
    sp = lambda t: t.reshape(B, L, 2, 10, H, W)
    ef = 5 * F.mse_loss(ap.sum(2), ag.sum(2)) + F.mse_loss(ap.sum((1, 2)), ag.sum((1, 2)))
    efs = 5 * F.mse_loss(sp(ap).sum(3), sp(ag).sum(3)) + F.mse_loss(sp(ap).sum((1, 3)), sp(ag).sum((1, 3)))
    out["ef"] = (ef + 2 * efs) / 2
    mp, mg = p > 0.01, g > 0.01
    out["compensation"] = F.mse_loss((p * mp).sum((2, 3)) / mp.sum((2, 3)).clamp(min=1),
                                     (g * mg).sum((2, 3)) / mg.sum((2, 3)).clamp(min=1))
    out["match"] = F.nll_loss(torch.log(F.softmax(p, dim=1)), g.argmax(dim=1))
    out["norml1"], out["norml2"] = torch.norm(p, p=1), torch.norm(p, p=2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--regimes", nargs="*", default=["sparse", "frac", "stress"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, B, Lq = 260, 346, a.B, a.L
    lib = hip.lib()
    st = hip.stream_ptr()
    rec = {"tool": "tools/voxlosses_bench.py", "device": torch.cuda.get_device_name(0), "shape": [B, Lq, 20, H, W],
           "stream_read_TBps": STREAM_BPS / 1e12, "regimes": {}}
    size = ctypes.sizeof(hip.VoxLossesStats)
    for regime in a.regimes:
        mk = lambda seed: torch.from_numpy(synth.synthetic_voxels(B * Lq, H, W, seed=seed, regime=regime)).cuda().reshape(
            B, Lq, 20, H, W)
        pred, gt = mk(1), mk(2)
        nbytes = 2 * 4 * pred.numel()
        r = {"algorithmic_bytes": nbytes}
        for name, terms in (("all", VL.ALL), ("no_match", tuple(t for t in VL.ALL if t != "match")), ("elementwise", ())):
            mask = VL.term_mask(terms)
            nb = lib.v2ce_voxlosses_workspace_bytes(B, Lq, 20, H, W, mask)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            out = torch.empty(B * size, dtype=torch.uint8, device="cuda")

            def call():
                hip.check(lib.v2ce_voxlosses(pred.data_ptr(), gt.data_ptr(), B, Lq, 20, H, W, mask, out.data_ptr(), size,
                                             ws.data_ptr(), nb, st), "v2ce_voxlosses")
            med, mn = timed(call, a.warmup, a.iters)
            r[f"{name}_ms"], r[f"{name}_ms_min"] = round(med, 4), round(mn, 4)
            r[f"{name}_TBps"] = round(nbytes / (med * 1e-3) / 1e12, 3)
            r[f"{name}_fraction_of_stream"] = round(nbytes / (med * 1e-3) / STREAM_BPS, 3)
            r[f"{name}_workspace_bytes"] = int(nb)
        s = VL.voxel_losses_batch(pred, gt).total()
        ours = {"mse": s.l2()[0], "pyramid": s.pyramid()[0], "pt": s.pt()[0], "ef": s.ef()[0],
                "compensation": s.compensation()[0], "match": s.match()[0], "norml1": s.norml1()[0],
                "norml2": s.norml2()[0]}
        with torch.no_grad():
            theirs = {k: float(v) for k, v in torch_terms(pred, gt).items()}
            r["max_rel_diff_to_torch_f32"] = max(abs(float(ours[k]) - theirs[k]) / abs(theirs[k]) for k in ours)
            assert r["max_rel_diff_to_torch_f32"] < 2e-3, (ours, theirs)      # torch's f32 norms are off by up to 5e-4
            med, mn = timed(lambda: torch_terms(pred, gt), 1, max(3, a.iters // 4))
        r["torch_ops_ms"], r["torch_ops_ms_min"] = round(med, 4), round(mn, 4)
        r["torch_ops_over_all"] = round(med / r["all_ms"], 2)
        rec["regimes"][regime] = r
        del pred, gt
        torch.cuda.empty_cache()
    rec.update({"iters": a.iters, "warmup": a.warmup, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
