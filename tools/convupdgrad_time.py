"""Time the input-gradient kernel of the last decoder block's conv1 and shortcut (v2ce_convup_dgrad) against the 32-channel
kernel behind it (v2ce_conv32_dgrad) and against torch's own route: conv3d input gradients (MIOpen, f32) into the
materialised 96-channel concat, the upsample backward, and the layout copies around them.  Prints one JSON line.

    python tools/convupdgrad_time.py [--iters 10] [--out profiles/NAME.json]

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
STEPS = [("updgrad_both", 240), ("updgrad_x0", 240), ("updgrad_x1", 240), ("conv32_dgrad", 240), ("torch_route", 420)]


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


def inputs():
    """-> weight [32, 96, 3, 3, 3], short_weight [32, 96], g1, gd [B, L, 2, H, pitch, 16] at the activation pitch."""
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    g = torch.Generator(device="cuda").manual_seed(1)
    w = 0.05 * torch.randn((32, 96, 3, 3, 3), generator=g, device="cuda")
    s = 0.1 * torch.randn((32, 96), generator=g, device="cuda")
    out = [w, s]
    for _ in range(2):
        t = torch.randn((B, L, 2, H, V2ce3d._pitch(W), 16), generator=g, device="cuda")
        t.lw, t.c16 = W, True
        out.append(t)
    return out


def step_updgrad(want, iters):
    import torch
    from v2ce_toolbox_amd import last_block
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    w, s, g1, gd = inputs()
    shape = {"x0": (B, L, 4, (H + 1) // 2, V2ce3d._pitch((W + 1) // 2), 16), "x1": tuple(g1.shape)}
    out = {n: torch.empty(shape[n], device="cuda") for n in want}
    med, best = median_ms(lambda: last_block.convup_dgrad(w, s, g1, gd, want=want, out=out), iters)
    flop = 2.0 * 32 * 28 * (64 * ("x0" in want) + 32 * ("x1" in want)) * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def step_conv32(iters):
    import torch
    from v2ce_toolbox_amd import last_conv
    w, _, up, _ = inputs()
    w32 = w[:, :32].contiguous()
    out = {"x": torch.empty_like(up)}
    med, best = median_ms(lambda: last_conv.conv32_dgrad(w32, None, up, want=("x",), out=out), iters)
    flop = 2.0 * 32 * 864 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def step_torch(iters):
    import torch
    w, s, g1, gd = inputs()
    s5 = s.view(32, 96, 1, 1, 1)
    H0, W0 = (H + 1) // 2, (W + 1) // 2

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def c16(p):                                              # and back: one layout copy (at the logical width)
        b, c, l, h, w_ = p.shape
        return p.reshape(b, c // 16, 16, l, h, w_).permute(0, 3, 1, 4, 5, 2).contiguous()

    def fn():
        dX = torch.nn.grad.conv3d_input((B, 96, L, H, W), w, planar(g1), padding=1) + \
            torch.nn.grad.conv3d_input((B, 96, L, H, W), s5, planar(gd))
        d0 = torch.ops.aten.upsample_nearest3d_backward(dX[:, :64].contiguous(), [L, H, W], [B, 64, L, H0, W0], None, None, None)
        return c16(d0), c16(dX[:, 64:])
    med, best = median_ms(fn, iters)
    flop = 2.0 * 32 * 96 * 28 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "concat_bytes": 96 * 4 * B * L * H * W}


def child(step, iters):
    if step == "updgrad_both":
        return step_updgrad(("x0", "x1"), iters)
    if step == "updgrad_x0":
        return step_updgrad(("x0",), iters)
    if step == "updgrad_x1":
        return step_updgrad(("x1",), iters)
    if step == "conv32_dgrad":
        return step_conv32(iters)
    return step_torch(iters)


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
    result = {"shape": [B, L, H, W], "peak_tf": PEAK_TF, "iters": a.iters, "flop_parity_with_conv32_dgrad": 3 * 28 / 27,
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
    if ms("updgrad_both") and ms("conv32_dgrad"):
        result["ratio_to_conv32_dgrad"] = ms("updgrad_both") / ms("conv32_dgrad")
        result["of_flop_parity"] = result["ratio_to_conv32_dgrad"] / (3 * 28 / 27)
    if ms("updgrad_both") and ms("torch_route"):
        result["speedup_over_torch_route"] = ms("torch_route") / ms("updgrad_both")
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all("error" not in v for v in result.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
