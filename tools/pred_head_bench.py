"""Rate of the trainable prediction head (v2ce_pred_head_fwd / v2ce_pred_head_grads, csrc/pred_head.hip) on 64 pairs of
346x260 as [4, 16, ., 260, 346]: 5.76 M positions, features channels-last-16 at pitch 352.

Timed (HIP events around each call, median of --iters after --warmup): the forward, the gradients without d_feat
(d_weight and d_bias, what a head fit runs) and the gradients with d_feat.  Algorithmic traffic per position, f32:
  forward              32 features read + Cout written
  gradients            32 features + Cout y + Cout upstream read = 72 floats at Cout = 20
  gradients + d_feat   the same + 32 written
"TBps" is those bytes over the call's time: a whole-call figure (the prep and finish kernels included), not a kernel's
share of peak.

The baseline is what a user would run without these kernels: torch autograd over ``relu(F.conv3d(x, w, b))`` on the
planar [B, 32, L, H, W] features on the same GPU -- forward alone, forward + backward for (w, b), and forward + backward
with x.requires_grad too; the backward's own time is the difference.  Before anything is timed the two are compared
(f32 torch against the f64-accumulating kernels: the largest difference relative to the largest value is recorded).
Prints one JSON line (--out writes it); whichever side is faster is recorded under "faster"."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from v2ce_toolbox_amd import hip, pred_head  # noqa: E402
from v2ce_toolbox_amd.v2ce_3d import V2ce3d  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 16, 260, 346], metavar=("B", "L", "H", "W"))
    ap.add_argument("--cout", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "pred_head_bench.py measures on a GPU; there is nothing to report without one"
    B, L, H, W = args.shape
    cout = args.cout
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.relu(torch.randn((B, 32, L, H, W), device=dev, generator=g))           # planar, as the reference's layer takes it
    w = torch.randn((cout, 32, 1, 1, 1), device=dev, generator=g) * 0.2
    b = torch.randn((cout,), device=dev, generator=g) * 0.1
    up = torch.randn((B, L, cout, H, W), device=dev, generator=g)
    pitch = V2ce3d._pitch(W)
    feat = torch.zeros((B, L, 2, H, pitch, 16), device=dev)
    feat[:, :, :, :, :W, :] = x.reshape(B, 2, 16, L, H, W).permute(0, 3, 1, 4, 5, 2)
    feat.lw, feat.c16 = W, True
    n = B * L * H * W
    rec = {"shape": [B, L, cout, H, W], "pitch": pitch, "positions": n, "warmup": args.warmup, "iters": args.iters,
           "device": torch.cuda.get_device_name(0), **hip.provenance()}

    y = pred_head.pred_head_forward(feat, w, b)
    outs = {"weight": torch.empty_like(w), "bias": torch.empty_like(b)}
    d_feat = torch.zeros_like(feat)
    calls = {
        "forward": (lambda: pred_head.pred_head_forward(feat, w, b, out=y), 32 + cout),
        "grads": (lambda: pred_head.pred_head_grads(feat, y, up, w, want=("weight", "bias"), out=outs), 32 + 2 * cout),
        "grads_d_feat": (lambda: pred_head.pred_head_grads(feat, y, up, w, want=("weight", "bias", "feat"),
                                                           out={**outs, "feat": d_feat}), 64 + 2 * cout),
    }
    for name, (fn, floats) in calls.items():
        med, lo, hi = timed(fn, args.warmup, args.iters)
        nbytes = 4.0 * floats * n
        rec[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "floats_per_position": floats, "algorithmic_GB": nbytes / 1e9,
                     "TBps": nbytes / (med * 1e-3) / 1e12}

    if not args.no_torch:
        F = torch.nn.functional
        up_t = up.permute(0, 2, 1, 3, 4)                                              # [B, cout, L, H, W] view
        wt, bt = w.clone().requires_grad_(), b.clone().requires_grad_()

        def fwd(xin):
            return torch.relu(F.conv3d(xin, wt, bt))

        def fwd_bwd(xin):
            wt.grad = bt.grad = None
            xin.grad = None
            fwd(xin).backward(up_t)

        xg = x.clone().requires_grad_()
        with torch.no_grad():
            yt = fwd(x)
        fwd_bwd(xg)
        full = pred_head.pred_head_grads(feat, y, up, w, want=("weight", "bias", "feat"), out={**outs, "feat": d_feat})
        rel = lambda a, t: float((a - t).abs().max() / t.abs().max())
        # torch's f32 convolution and the f64 sums disagree on the sign of a pre-activation next to zero at a few units;
        # there the two masks differ and so does d_feat of that position (by upstream * weight, nothing small): counted,
        # and left out of the d_feat comparison
        flipped = (y.permute(0, 2, 1, 3, 4) > 0) != (yt > 0)                              # [B, cout, L, H, W]
        same = ~flipped.any(dim=1)[:, :, None, :, :, None]                                # [B, L, 1, H, W, 1]
        ours_f = full["feat"][:, :, :, :, :W, :] * same
        torch_f = xg.grad.reshape(B, 2, 16, L, H, W).permute(0, 3, 1, 4, 5, 2) * same
        rec["vs_torch_f32"] = {
            "y": rel(y.permute(0, 2, 1, 3, 4), yt), "d_weight": rel(full["weight"], wt.grad), "d_bias": rel(full["bias"], bt.grad),
            "d_feat_where_masks_agree": rel(ours_f, torch_f), "units_with_flipped_mask": int(flipped.sum()),
            "units": int(flipped.numel())}
        del ours_f, torch_f, same, flipped
        del yt
        t = {}
        with torch.no_grad():
            t["forward"] = timed(lambda: fwd(x), args.warmup, args.iters)
        t["forward_backward"] = timed(lambda: fwd_bwd(x), args.warmup, args.iters)
        t["forward_backward_d_feat"] = timed(lambda: fwd_bwd(xg), args.warmup, args.iters)
        rec["torch"] = {k: {"ms": v[0], "ms_min": v[1], "ms_max": v[2]} for k, v in t.items()}
        rec["torch"]["backward_ms"] = t["forward_backward"][0] - t["forward"][0]
        rec["torch"]["backward_d_feat_ms"] = t["forward_backward_d_feat"][0] - t["forward"][0]
        pairs = {"forward": (rec["forward"]["ms"], t["forward"][0]),
                 "grads": (rec["grads"]["ms"], rec["torch"]["backward_ms"]),
                 "grads_d_feat": (rec["grads_d_feat"]["ms"], rec["torch"]["backward_d_feat_ms"])}
        rec["faster"] = {k: ("hip" if a < c else "torch") for k, (a, c) in pairs.items()}
        rec["torch_over_hip"] = {k: c / a for k, (a, c) in pairs.items()}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
