"""Time the weight-gradient kernel of UNet.decoders[2].conv1 and its shortcut (v2ce_convupn_wgrad at 128 + 64 -> 64, all three
outputs) at that layer's shape [1, 16, 130, 173] against the same kernel through the 64 + 32 -> 32 entry (v2ce_convup_wgrad) at
the last block's shape [1, 16, 260, 346] -- the two calls execute the same number of MFMA flops, 4 times the channel products over a
quarter of the positions, on almost the same tile count per workgroup --, against torch's own route (conv3d weight gradients
on the materialised upsample + concat in planar f32, MIOpen, plus the layout copies a channels-last-16 caller pays), and one
fit_dec2_block step next to one fit_dec2_conv step at the default frame size.  Prints one JSON line.

    python tools/convupngrad_time.py [--iters 10] [--out profiles/NAME.json]

One process.  Kernel times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts 2 * cout * (c0 + c1) *
28 * positions (27 taps and the shortcut) against the 155 TF peak of the exact-f32 MFMA."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
B, L = 1, 16
DEC2 = (130, 173)
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


def act(g, c, h, w):
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    t = torch.randn((B, L, c // 16, h, V2ce3d._pitch(w), 16), generator=g, device="cuda")
    t.lw, t.c16 = w, True
    return t


def entry(med, best, cin, cout, h, w):
    flop = 2.0 * cout * cin * 28 * B * L * h * w
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF}


def tensors(g, c0, c1, cout, h, w):
    return act(g, c0, (h + 1) // 2, (w + 1) // 2), act(g, c1, h, w), act(g, cout, h, w), act(g, cout, h, w)


def kernels(iters):
    import torch
    from v2ce_toolbox_amd import dec2_block, last_block
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for (c0, c1, cout), (h, w), fn, tag in (((128, 64, 64), DEC2, dec2_block.convupn_wgrad, "convupn_wgrad_dec2"),
                                            ((64, 32, 32), FRAME, last_block.convup_wgrad, "convup_wgrad_dec3"),
                                            ((64, 32, 32), FRAME, dec2_block.convupn_wgrad, "convupn_wgrad_dec3")):
        x0, x1, g1, gd = tensors(g, c0, c1, cout, h, w)
        o = {"weight": torch.empty((cout, c0 + c1, 3, 3, 3), device="cuda"), "short": torch.empty((cout, c0 + c1), device="cuda"),
             "short_bias": torch.empty(cout, device="cuda")}
        out[tag] = entry(*median_ms(lambda: fn(x0, x1, g1, gd, out=o), iters), c0 + c1, cout, h, w)
    return out


def torch_route(iters):
    import torch
    g = torch.Generator(device="cuda").manual_seed(2)
    h, w = DEC2
    x0, x1, g1, gd = tensors(g, 128, 64, 64, h, w)

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def wgrad():
        X = torch.cat([torch.nn.functional.interpolate(planar(x0), size=(L, h, w), mode="nearest"), planar(x1)], dim=1)
        s = planar(gd)
        return (torch.nn.grad.conv3d_weight(X, (64, 192, 3, 3, 3), planar(g1), padding=1),
                torch.nn.grad.conv3d_weight(X, (64, 192, 1, 1, 1), s), s.sum(dim=(0, 2, 3, 4)))
    return {"torch_wgrad_dec2": entry(*median_ms(wgrad, iters), 192, 64, h, w)}


def fit_steps(iters):
    """One optimizer step of fit_dec2_block and of fit_dec2_conv at the default frame size, inputs cached: wall time per step
    from two fits of different lengths (the cached forward of the frozen trunk cancels)."""
    import time

    import numpy as np
    import torch
    from v2ce_toolbox_amd import finetune, synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    fr = synth.synthetic_frames(L + 1, *FRAME, seed=3).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).cuda()
    out = {}
    for name, fit in (("fit_dec2_conv_step", finetune.fit_dec2_conv), ("fit_dec2_block_step", finetune.fit_dec2_block)):
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
    result = {"dec2_shape": [B, L, *DEC2], "frame": list(FRAME), "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
    result.update(kernels(a.iters))
    result.update(torch_route(a.iters))
    if not a.no_fit:
        result.update(fit_steps(a.iters))
    ms = lambda k: result[k]["ms"]
    result["dec2_ratio_to_convup_wgrad_dec3"] = ms("convupn_wgrad_dec2") / ms("convup_wgrad_dec3")
    result["convupn_ratio_to_convup_at_dec3"] = ms("convupn_wgrad_dec3") / ms("convup_wgrad_dec3")
    result["speedup_over_torch"] = ms("torch_wgrad_dec2") / ms("convupn_wgrad_dec2")
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
