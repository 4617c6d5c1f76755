"""Time of the image-gradient input channel and of the three-channel head on the flagship shape: --packets x --seq_len
pairs of 260 x 346 (default 4 x 16 = 64 pairs).

  * image_units_batch (v2ce_image_units_grad, csrc/imgrad.hip: uint8 frames -> f32 [S, L, 3, H, W]) and the gradient /
    blur kernel alone (v2ce_image_grad_batch), against the reference's formula as torch device ops on the same frames
    (image_derivative.py:38-75 and event_pack_dataset.py:66-73 restated: two F.conv2d Sobel passes per frame, sqrt,
    maximum, reflect pad and a depthwise 11 x 11 conv2d, the packet maximum, Normalize, cat);
  * the head convolution of a three-channel V2ce3d at [S, L, 3, 260, 346]: the split-half kernel
    (v2ce_conv3d_head_f16x2, C0 = 3) against the generic exact-f32 launch that such a weight took before.

HIP events (median over --iters windows of --reps calls, after --warmup).  The record states the bytes each call must
move next to its time.  Prints one JSON line (--out writes it).  A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from v2ce_toolbox_amd import hip  # noqa: E402
from v2ce_toolbox_amd import image_derivative as ID  # noqa: E402
from v2ce_toolbox_amd import synth  # noqa: E402


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


def torch_units(frames, taps2d, sobel_x, sobel_y, mean, std):
    """The reference's steps as device ops: uint8 [S, L+1, H, W] -> f32 [S, L, 3, H, W]."""
    S, L1, H, W = frames.shape
    x = frames.float() / 255
    units = torch.stack([x[:, :-1], x[:, 1:]], dim=2)                       # [S, L, 2, H, W]
    flat = units.reshape(S * (L1 - 1), 2, H, W)
    grads = []
    for c in range(2):
        img = flat[:, c:c + 1]
        gx, gy = F.conv2d(img, sobel_x, padding=1), F.conv2d(img, sobel_y, padding=1)
        grads.append(torch.sqrt(gx ** 2 + gy ** 2))
    merged = torch.maximum(grads[0], grads[1])
    r = taps2d.shape[-1] // 2
    blur = F.conv2d(F.pad(merged, [r, r, r, r], mode="reflect"), taps2d).reshape(S, L1 - 1, 1, H, W)
    blur = blur / blur.amax(dim=(1, 2, 3, 4), keepdim=True)
    return torch.cat([(units - mean) / std, blur], dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=4)
    ap.add_argument("--seq_len", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--commit", type=str, default=None, help="recorded as given (the GPU box may have no .git)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, S, L = 260, 346, a.packets, a.seq_len
    P = S * L
    frames = torch.from_numpy(np.stack([synth.synthetic_frames(L + 1, H, W, seed=7 + s) for s in range(S)])).cuda()
    lib, st = hip.lib(), hip.stream_ptr()
    taps = ID.gaussian_taps()
    nb = lib.v2ce_image_grad_workspace_bytes(S, L, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    units = torch.empty((S, L, 3, H, W), device="cuda")
    blur = torch.empty((S, L, H, W), device="cuda")
    gmax = torch.empty(S, device="cuda")
    rec = {"tool": "tools/image_grad_bench.py", "device": torch.cuda.get_device_name(0), "packets": S, "seq_len": L, "pairs": P,
           "H": H, "W": W, "kernel_size": 11, "sigma": 3, "commit": a.commit,
           # the gradient kernel reads each pair's two frames (halo re-reads come from L2) and writes the blur; the units kernel reads the
           # two frames and the blur again and writes three planes
           "grad_bytes": P * H * W * (2 + 4), "units_bytes": P * H * W * (2 + 4) + P * H * W * (2 + 4 + 12)}

    def units_call():
        hip.check(lib.v2ce_image_units_grad(frames.data_ptr(), S, L, H, W, ID._fp(taps), 11, 0.153, 0.165, units.data_ptr(),
                                            gmax.data_ptr(), ws.data_ptr(), nb, st), "v2ce_image_units_grad")

    def grad_call():
        hip.check(lib.v2ce_image_grad_batch(frames.data_ptr(), S, L, H, W, ID._fp(taps), 11, blur.data_ptr(), gmax.data_ptr(), st),
                  "v2ce_image_grad_batch")

    for name, call, nbytes in (("units", units_call, rec["units_bytes"]), ("grad", grad_call, rec["grad_bytes"])):
        med, mn = timed(call, a.warmup, a.iters, a.reps)
        rec[f"device_{name}_ms"], rec[f"device_{name}_ms_min"] = round(med, 4), round(mn, 4)
        rec[f"device_{name}_GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)
    med, mn = timed(lambda: ID.image_units_batch(frames), a.warmup, a.iters, a.reps)
    rec["api_units_ms"], rec["api_units_ms_min"] = round(med, 4), round(mn, 4)

    t1 = torch.from_numpy(taps).cuda()
    taps2d = torch.mm(t1[:, None], t1[None, :])[None, None]
    sobel_x = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=torch.float32, device="cuda").view(1, 1, 3, 3)
    sobel_y = sobel_x.permute(0, 1, 3, 2).contiguous()
    want = torch_units(frames, taps2d, sobel_x, sobel_y, 0.153, 0.165)
    units_call()
    torch.cuda.synchronize()
    rec["max_abs_diff_to_torch_ops"] = float((units - want).abs().max().item())
    med, mn = timed(lambda: torch_units(frames, taps2d, sobel_x, sobel_y, 0.153, 0.165), a.warmup, max(3, a.iters // 4), 2)
    rec["torch_ops_ms"], rec["torch_ops_ms_min"] = round(med, 4), round(mn, 4)
    rec["speedup_units_over_torch_ops"] = round(med / rec["device_units_ms"], 2)

    # the three-channel head: split-half kernel against the generic exact-f32 launch of the same weight
    from v2ce_toolbox_amd.v2ce_3d import BASE, V2ce3d
    sd = synth.make_state_dict(0)
    g = torch.Generator().manual_seed(2024)
    sd["UNet.head.conv3d.weight"] = torch.randn(32, 3, 3, 3, 3, generator=g) * float(sd["UNet.head.conv3d.weight"].std())
    m = V2ce3d(in_channels=3)
    m.load_state_dict(sd)
    m = m.eval().cuda()
    m._prepare()
    prep = m._prep
    assert prep["head_split"] is not None
    prep["absmax"] = torch.zeros((64, S, 2), dtype=torch.float32, device="cuda")
    x = units

    def split_head():
        m._slot = 0
        return m._head_split(x, *prep["head_split"])

    def generic_head():
        m._slot = 0
        return m._conv(x, None, *prep["head"], BASE, 3, 1, hip.ACT_LEAKY, track=True)

    a_, b_ = V2ce3d.to_planar(split_head()), V2ce3d.to_planar(generic_head())
    rec["head_max_abs_diff_split_vs_generic"] = float((a_ - b_).abs().max().item())
    del a_, b_
    head_bytes = P * H * W * 4 * (3 + 32)
    for name, call in (("head_split_c3", split_head), ("head_generic_f32_c3", generic_head)):
        med, mn = timed(call, a.warmup, a.iters, 5)
        rec[f"{name}_ms"], rec[f"{name}_ms_min"] = round(med, 4), round(mn, 4)
        rec[f"{name}_GBps"] = round(head_bytes / (med * 1e-3) / 1e9, 1)
    rec["head_bytes"] = head_bytes
    rec["speedup_head_split_over_generic"] = round(rec["head_generic_f32_c3_ms"] / rec["head_split_c3_ms"], 2)
    rec.update({"iters": a.iters, "reps": a.reps, "warmup": a.warmup, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
