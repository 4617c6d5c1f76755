"""Time the 64-channel gradient kernels of UNet.decoders[2].conv2 (v2ce_convn_wgrad, v2ce_convn_dgrad) at that layer's
shape [1, 16, 130, 173] against the same kernels at 32 -> 32 through the 32-channel entries (v2ce_conv32_wgrad,
v2ce_conv32_dgrad) at the same positions, against torch's own route (conv3d weight / input gradients on planar f32, MIOpen, plus the layout copies a
channels-last-16 caller pays), and one fit_dec2_conv step next to one fit_last_block step at the default frame size.
Prints one JSON line.

    python tools/convngrad_time.py [--iters 10] [--out profiles/NAME.json]

One process.  Kernel times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts 2 * cout * cin * 27 *
positions per gradient against the 155 TF peak of the exact-f32 MFMA.  Flop parity of a 64 -> 64 call with the 32 -> 32 one
at the same positions is 4 times its time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
B, L, H, W = 1, 16, 130, 173
FRAME = (260, 346)


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


def act(g, c):
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    t = torch.randn((B, L, c // 16, H, V2ce3d._pitch(W), 16), generator=g, device="cuda")
    t.lw, t.c16 = W, True
    return t


def entry(med, best, cin, cout):
    flop = 2.0 * cout * cin * 27 * B * L * H * W
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def kernels(iters):
    import torch
    from v2ce_toolbox_amd import dec2_conv, last_conv
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for c, wg, dg, tag in ((64, dec2_conv.convn_wgrad, dec2_conv.convn_dgrad, "convn_64"),
                           (32, last_conv.conv32_wgrad, last_conv.conv32_dgrad, "conv32")):
        x, y, up = act(g, c), act(g, c), act(g, c)
        w = 0.05 * torch.randn((c, c, 3, 3, 3), generator=g, device="cuda")
        ow = {"weight": torch.empty_like(w), "shift": torch.empty(c, device="cuda")}
        ox = {"x": torch.empty_like(up), "res": torch.empty_like(up)}
        out[tag + "_wgrad"] = entry(*median_ms(lambda: wg(x, y, up, out=ow), iters), c, c)
        out[tag + "_dgrad"] = entry(*median_ms(lambda: dg(w, y, up, out=ox), iters), c, c)
        out[tag + "_dgrad_x_alone"] = entry(*median_ms(lambda: dg(w, y, up, want=("x",), out={"x": ox["x"]}), iters), c, c)
    return out


def torch_route(iters):
    import torch
    g = torch.Generator(device="cuda").manual_seed(2)
    x, y, up = act(g, 64), act(g, 64), act(g, 64)
    w = 0.05 * torch.randn((64, 64, 3, 3, 3), generator=g, device="cuda")

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def c16(p):                                              # and back: one layout copy (at the logical width)
        b, c, l, h, w_ = p.shape
        return p.reshape(b, c // 16, 16, l, h, w_).permute(0, 3, 1, 4, 5, 2).contiguous()

    def masked():
        return torch.where(planar(y) > 0, planar(up), torch.zeros((), device="cuda"))

    def wgrad():
        m = masked()
        return torch.nn.grad.conv3d_weight(planar(x), w.shape, m, padding=1), m.sum(dim=(0, 2, 3, 4))

    def dgrad():
        m = masked()
        return c16(torch.nn.grad.conv3d_input((B, 64, L, H, W), w, m, padding=1)), c16(m)
    return {"torch_wgrad": entry(*median_ms(wgrad, iters), 64, 64), "torch_dgrad": entry(*median_ms(dgrad, iters), 64, 64)}


def fit_steps(iters):
    """One optimizer step of fit_dec2_conv and of fit_last_block at the default frame size, inputs cached: wall time per step
    from two fits of different lengths (the cached forward of the frozen trunk cancels)."""
    import time

    import numpy as np
    import torch
    from v2ce_toolbox_amd import finetune, synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    fr = synth.synthetic_frames(L + 1, *FRAME, seed=3).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).cuda()
    out = {}
    for name, fit in (("fit_last_block_step", finetune.fit_last_block), ("fit_dec2_conv_step", finetune.fit_dec2_conv)):
        def run(steps):
            m = V2ce3d()
            m.load_state_dict(synth.make_state_dict(0))
            m = m.eval().cuda()
            gt = m(x).clone() * 0.9
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit(m, x, gt, steps=steps, lr=1e-6, optimizer="sgd")
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run(2)                                               # warm-up: allocator, kernel loads
        few, many = 2, 2 + max(iters // 2, 3)
        a, b = run(few), run(many)
        out[name] = {"ms": (b - a) / (many - few) * 1e3, "steps_timed": many - few}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_fit", action="store_true", help="kernels and torch's route only")
    a = ap.parse_args()
    from v2ce_toolbox_amd import hip
    result = {"shape": [B, L, H, W], "frame": list(FRAME), "peak_tf": PEAK_TF, "iters": a.iters, "flop_parity_with_conv32": 4.0,
              **hip.provenance()}
    result.update(kernels(a.iters))
    result.update(torch_route(a.iters))
    if not a.no_fit:
        result.update(fit_steps(a.iters))
    ms = lambda k: result[k]["ms"]
    for kind in ("wgrad", "dgrad"):
        result[f"{kind}_ratio_to_conv32"] = ms(f"convn_64_{kind}") / ms(f"conv32_{kind}")
        result[f"{kind}_of_flop_parity"] = result[f"{kind}_ratio_to_conv32"] / 4.0
        result[f"{kind}_speedup_over_torch"] = ms(f"torch_{kind}") / ms(f"convn_64_{kind}")
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
