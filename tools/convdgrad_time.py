"""Time the input-gradient kernel of the last decoder convolution (v2ce_conv32_dgrad) against torch's own conv3d input
gradient (MIOpen, f32) on the same data -- planar, with and without the two layout copies a channels-last-16 caller would
pay -- and against the project's exact-f32 forward launch of the same layer at the same shape, which issues the same number
of f32 MFMAs: the yardstick (csrc/conv3d.hip, untouched by the input-gradient work).  Prints one JSON line.

    python tools/convdgrad_time.py [--iters 10] [--out profiles/NAME.json]

Every GPU step runs in a child process of its own under a time limit; after a step that fails or runs out of time no
further step is started.  Kernel times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts the
2 * 32 * 864 * positions flop of the layer's GEMM against the 157 TF peak of the exact-f32 MFMA."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.0
B, H, W, L = 1, 260, 346, 16
FLOP = 2.0 * 32 * 864 * B * L * H * W
STEPS = [("dgrad", 240), ("forward_f32", 240), ("torch", 420)]


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


def rate(med, best):
    return {"ms": med, "ms_min": best, "tflops": FLOP / med / 1e9, "of_f32_mfma_peak": FLOP / med / 1e9 / PEAK_TF}


def c16_inputs():
    """-> (y, upstream) channels-last-16 at the activation pitch, and a weight of the layer's size."""
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    g = torch.Generator(device="cuda").manual_seed(1)
    pitch = V2ce3d._pitch(W)
    y = torch.randn((B, L, 2, H, pitch, 16), generator=g, device="cuda").clamp_(min=0)
    up = torch.randn((B, L, 2, H, pitch, 16), generator=g, device="cuda")
    for t in (y, up):
        t.lw, t.c16 = W, True
    w = (torch.randn((32, 32, 3, 3, 3), generator=g, device="cuda") * 0.05).contiguous()
    return y, up, w


def step_dgrad(iters):
    import torch
    from v2ce_toolbox_amd import last_conv
    y, up, w = c16_inputs()
    out = {"x": torch.empty_like(up), "res": torch.empty_like(up)}
    res = {"both": rate(*median_ms(lambda: last_conv.conv32_dgrad(w, y, up, out=out), iters))}
    res["x_only"] = rate(*median_ms(lambda: last_conv.conv32_dgrad(w, y, up, want=("x",), out={"x": out["x"]}), iters))
    med, best = median_ms(lambda: last_conv.conv32_dgrad(w, y, up, want=("res",), out={"res": out["res"]}), iters)
    res["res_only"] = {"ms": med, "ms_min": best}
    return res


def step_forward(iters):
    """conv2 + bn2 + residual + relu of the last decoder block as LastConv's forward launches it on the exact-f32 path."""
    import torch
    from v2ce_toolbox_amd import hip, synth
    from v2ce_toolbox_amd.last_conv import _planar_pitched
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d(precision="f32")
    m.load_state_dict(synth.make_state_dict(0))
    m = m.eval().to("cuda:0")
    y, up, w = c16_inputs()
    with torch.no_grad():
        m._prepare()
        t, res = _planar_pitched(y), _planar_pitched(up)
        packed = m._pack(w, split=False)
        scale, shift = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
        fn = lambda: m._conv(t, None, packed, scale, shift, 32, 3, 1, hip.ACT_RELU, residual=res, split=False)
        return rate(*median_ms(fn, iters))


def step_torch(iters):
    import torch
    y, up, w = c16_inputs()
    m16 = torch.where(y > 0, up, torch.zeros_like(up))                 # (the mask is applied beforehand: not timed)
    m16.lw, m16.c16 = W, True
    del y, up
    # channels-last-16 [B, L, 2, H, pitch, 16] -> torch's [B, 32, L, H, W] and back, one full-size copy each
    planar = lambda t: t[:, :, :, :, :W, :].permute(0, 2, 5, 1, 3, 4).reshape(B, 32, L, H, W)
    c16 = lambda d: d.view(B, 2, 16, L, H, W).permute(0, 3, 1, 4, 5, 2).contiguous()
    m = planar(m16)
    assert m.is_contiguous()
    grad = lambda mm: torch.nn.grad.conv3d_input((B, 32, L, H, W), w, mm, padding=1)
    res = {"planar": rate(*median_ms(lambda: grad(m), iters))}

    def with_copies():
        return c16(grad(planar(m16)))
    res["with_layout_copies"] = rate(*median_ms(with_copies, iters))
    res["mask_applied_beforehand"] = True
    return res


def child(step, iters):
    return {"dgrad": step_dgrad, "forward_f32": step_forward, "torch": step_torch}[step](iters)


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
    result = {"shape": [B, L, H, W], "gflop": FLOP / 1e9, "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
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
    if "both" in result.get("dgrad", {}):
        ms = result["dgrad"]["x_only"]["ms"]
        if "ms" in result.get("forward_f32", {}):
            result["dgrad_over_forward_f32"] = ms / result["forward_f32"]["ms"]
        if "planar" in result.get("torch", {}):
            result["speedup_over_torch_planar"] = result["torch"]["planar"]["ms"] / ms
            result["speedup_over_torch_with_layout_copies"] = result["torch"]["with_layout_copies"]["ms"] / ms
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all("error" not in v for v in result.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
