"""Time the weight-gradient kernel of the last decoder block's conv1 and shortcut (v2ce_convup_wgrad) against the 32-channel
kernel behind it (v2ce_conv32_wgrad) and against torch's own conv3d weight gradient (MIOpen, f32) on the materialised
upsample + concat, and one fit_last_block step against one fit_tail_norms step.  Prints one JSON line.

    python tools/convupgrad_time.py [--iters 10] [--out profiles/NAME.json]

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time no
further step is started.  Kernel times are medians of HIP-event intervals after three warm-up calls at [1, 16, 260, 346];
TFLOP/s counts the 2 * 32 * 96 * 28 * positions flop of the two gradients' GEMMs against the 155 TF peak of the exact-f32
MFMA.  Flop parity with the 32-channel kernel is 3 channel groups x 28 / 27 units = 3.11 times its time."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
B, H, W, L = 1, 260, 346, 16
STEPS = [("upwgrad_all", 240), ("upwgrad_weight", 240), ("conv32_wgrad", 240), ("torch_materialised", 420),
         ("torch_with_upsample_and_copies", 420), ("fit", 420)]


def median_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def c16_inputs():
    """-> x0 [B, L, 4, H0, pitch0, 16], x1, g1, gd [B, L, 2, H, pitch, 16] at the activation pitches."""
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    g = torch.Generator(device="cuda").manual_seed(1)
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    x0 = torch.randn((B, L, 4, H0, V2ce3d._pitch(W0), 16), generator=g, device="cuda")
    x0.lw, x0.c16 = W0, True
    out = [x0]
    for _ in range(3):
        t = torch.randn((B, L, 2, H, V2ce3d._pitch(W), 16), generator=g, device="cuda")
        t.lw, t.c16 = W, True
        out.append(t)
    return out


def step_upwgrad(want, iters):
    import torch
    from v2ce_toolbox_amd import last_block
    x0, x1, g1, gd = c16_inputs()
    out = {n: torch.empty(last_block._SHAPES[n], device="cuda") for n in want}
    med, best = median_ms(lambda: last_block.convup_wgrad(x0, x1, g1, gd, want=want, out=out), iters)
    flop = 2.0 * 32 * 96 * (27 * ("weight" in want) + ("short" in want)) * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def step_conv32(iters):
    import torch
    from v2ce_toolbox_amd import last_conv
    _, x, y, up = c16_inputs()
    out = {"weight": torch.empty((32, 32, 3, 3, 3), device="cuda")}
    med, best = median_ms(lambda: last_conv.conv32_wgrad(x, None, up, want=("weight",), out=out), iters)
    flop = 2.0 * 32 * 864 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def step_torch(with_copies, iters):
    import torch
    import torch.nn.functional as F
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    x0, x1, g1, _ = c16_inputs()

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def concat():
        return torch.cat([F.interpolate(planar(x0), size=(L, H, W), mode="nearest"), planar(x1)], dim=1)
    g = planar(g1)
    if with_copies:
        fn = lambda: torch.nn.grad.conv3d_weight(concat(), (32, 96, 3, 3, 3), planar(g1), padding=1)
    else:
        X = concat()
        fn = lambda: torch.nn.grad.conv3d_weight(X, (32, 96, 3, 3, 3), g, padding=1)
    med, best = median_ms(fn, iters)
    flop = 2.0 * 32 * 96 * 27 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "concat_bytes": 96 * 4 * B * L * H * W}


def step_fit(iters):
    import time
    import numpy as np
    import torch
    from v2ce_toolbox_amd import finetune, synth
    from v2ce_toolbox_amd.pred_head import PredHead, pred_head_forward
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d

    def model():
        m = V2ce3d()
        m.load_state_dict(synth.make_state_dict(0))
        return m.eval().to("cuda:0")
    fr = synth.synthetic_frames(L + 1, H, W, seed=3).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).cuda()
    m = model()
    head = PredHead.from_model(m)
    gt = pred_head_forward(m.forward_features(x), (head.weight.detach() * 1.1).contiguous(), head.bias.detach())
    res = {}
    for name, fit in (("fit_tail_norms", finetune.fit_tail_norms), ("fit_last_block", finetune.fit_last_block)):
        fit(model(), x, gt, steps=2, lr=1e-6)                       # warm-up: code objects, allocator
        t = {}
        for steps in (2, 2 + iters):
            mm = model()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit(mm, x, gt, steps=steps, lr=1e-6)
            torch.cuda.synchronize()
            t[steps] = time.perf_counter() - t0
        res[name + "_step_ms"] = (t[2 + iters] - t[2]) / iters * 1e3     # (wall clock: host work of a step included)
    return res


def child(step, iters):
    if step == "upwgrad_all":
        return step_upwgrad(("weight", "short", "short_bias"), iters)
    if step == "upwgrad_weight":
        return step_upwgrad(("weight",), iters)
    if step == "conv32_wgrad":
        return step_conv32(iters)
    if step.startswith("torch_"):
        return step_torch(step != "torch_materialised", iters)
    return step_fit(iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(child(a.step, a.iters)))
        return 0
    from v2ce_toolbox_amd import hip
    result = {"shape": [B, L, H, W], "peak_tf": PEAK_TF, "iters": a.iters, "flop_parity_with_conv32_wgrad": 3 * 28 / 27,
              **hip.provenance()}
    for step, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"no result within {limit} s"}
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            result[step] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}
            break
        result[step] = json.loads(line[-1][7:])
    ms = lambda k: result.get(k, {}).get("ms")
    if ms("upwgrad_all") and ms("conv32_wgrad"):
        result["ratio_to_conv32_wgrad"] = ms("upwgrad_all") / ms("conv32_wgrad")
        result["weight_alone_ratio_to_conv32_wgrad"] = ms("upwgrad_weight") / ms("conv32_wgrad") if ms("upwgrad_weight") else None
    for k in ("torch_materialised", "torch_with_upsample_and_copies"):
        if ms("upwgrad_weight") and ms(k):
            result[f"speedup_over_{k}"] = ms(k) / ms("upwgrad_weight")
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all("error" not in v for v in result.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
