"""Time the weight-gradient kernel of the last decoder convolution (v2ce_conv32_wgrad) against torch's own conv3d weight
gradient (MIOpen, f32) on the same tensors, and one fit_tail step against one fit_head step.  Prints one JSON line.

    python tools/convgrad_time.py [--iters 10] [--out profiles/NAME.json]

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time no
further step is started.  Kernel times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts the
2 * 32 * 864 * positions flop of the gradient's GEMM against the 155 TF peak of the exact-f32 MFMA."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
H, W, L = 260, 346, 16
STEPS = [("wgrad_b1", 240), ("torch_b1", 420), ("wgrad_b4", 240), ("torch_b4", 420), ("fit", 420)]


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


def c16_inputs(B):
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    g = torch.Generator(device="cuda").manual_seed(B)
    pitch = V2ce3d._pitch(W)
    out = []
    for i in range(3):
        t = torch.randn((B, L, 2, H, pitch, 16), generator=g, device="cuda")
        if i < 2:
            t.clamp_(min=0)
        t.lw, t.c16 = W, True
        out.append(t)
    return out


def step_wgrad(B, iters):
    import torch
    from v2ce_toolbox_amd import last_conv
    x, y, up = c16_inputs(B)
    out = {"weight": torch.empty((32, 32, 3, 3, 3), device="cuda"), "shift": torch.empty(32, device="cuda")}
    med, best = median_ms(lambda: last_conv.conv32_wgrad(x, y, up, out=out), iters)
    flop = 2.0 * 32 * 864 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def step_torch(B, iters):
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    x, y, up = (V2ce3d.to_planar(t).permute(0, 2, 1, 3, 4).contiguous() for t in c16_inputs(B))   # [B, 32, L, H, W]
    m = torch.where(y > 0, up, torch.zeros_like(up))
    del y, up
    fn = lambda: torch.nn.grad.conv3d_weight(x, (32, 32, 3, 3, 3), m, padding=1)
    med, best = median_ms(fn, iters)
    flop = 2.0 * 32 * 864 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "mask_applied_beforehand": True}


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
    for name, fit in (("fit_head", finetune.fit_head), ("fit_tail", finetune.fit_tail)):
        fit(model(), x, gt, steps=2, lr=1e-4)                       # warm-up: code objects, allocator, MIOpen-free paths
        t = {}
        for steps in (2, 2 + iters):
            mm = model()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit(mm, x, gt, steps=steps, lr=1e-4)
            torch.cuda.synchronize()
            t[steps] = time.perf_counter() - t0
        res[name + "_step_ms"] = (t[2 + iters] - t[2]) / iters * 1e3     # (wall clock: host work of a step included)
    return res


def child(step, iters):
    if step.startswith("wgrad_b"):
        return step_wgrad(int(step[7:]), iters)
    if step.startswith("torch_b"):
        return step_torch(int(step[7:]), iters)
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
    result = {"shape": [L, H, W], "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
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
    for b in (1, 4):
        if "ms" in result.get(f"wgrad_b{b}", {}) and "ms" in result.get(f"torch_b{b}", {}):
            result[f"speedup_over_torch_b{b}"] = result[f"torch_b{b}"]["ms"] / result[f"wgrad_b{b}"]["ms"]
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all("error" not in v for v in result.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
