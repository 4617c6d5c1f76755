"""Time the input-gradient kernel of UNet.decoders[2].conv1 and its shortcut (v2ce_convupn_dgrad at 128 + 64 -> 64: both
outputs, then each alone) at that layer's shape [1, 16, 130, 173] against the same kernel template through the 64 + 32 -> 32
entry (v2ce_convup_dgrad) at the last block's shape [1, 16, 260, 346] -- the two calls execute the same number of MFMA flops, 4
times the channel products over a quarter of the positions --, against torch's own route for the 192 -> 64 case (conv3d input
gradients of both convolutions on the materialised planar concat, MIOpen f32, the upsample backward, and the layout copies a
channels-last-16 caller pays), and one Dec2BlockThrough -> LastBlock -> PredHead forward + backward step next to the same
step with Dec2Block at the default frame size: the difference is the cost of the new gradient inside a training step.
Prints one JSON line.

    python tools/convupndgrad_time.py [--iters 10] [--out profiles/NAME.json]

One process.  Times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts 2 * cout * (c0 + c1) * 28 *
positions (27 taps and the shortcut; with one output alone, that output's channels only) against the 155 TF peak of the
exact-f32 MFMA."""
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


def weights(g, c0, c1, cout):
    import torch
    return (0.05 * torch.randn((cout, c0 + c1, 3, 3, 3), generator=g, device="cuda"),
            0.1 * torch.randn((cout, c0 + c1), generator=g, device="cuda"))


def kernels(iters):
    import torch
    from v2ce_toolbox_amd import dec2_block, last_block
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for (c0, c1, cout), (h, w), fn, tag, wants in (
            ((128, 64, 64), DEC2, dec2_block.convupn_dgrad, "convupn_dgrad_dec2", (("x0", "x1"), ("x0",), ("x1",))),
            ((64, 32, 32), FRAME, last_block.convup_dgrad, "convup_dgrad_dec3", (("x0", "x1"),)),
            ((64, 32, 32), FRAME, dec2_block.convupn_dgrad, "convupn_dgrad_dec3", (("x0", "x1"),))):
        (wt, sw), g1, gd = weights(g, c0, c1, cout), act(g, cout, h, w), act(g, cout, h, w)
        shape = {"x0": (B, L, c0 // 16, (h + 1) // 2, V2ce3d._pitch((w + 1) // 2), 16), "x1": (B, L, c1 // 16, h, g1.shape[4], 16)}
        for want in wants:
            o = {n: torch.empty(shape[n], device="cuda") for n in want}
            kw = {"c0": c0} if fn is dec2_block.convupn_dgrad and "x0" not in want else {}
            cin = c0 * ("x0" in want) + c1 * ("x1" in want)
            name = tag + ("" if len(want) == 2 else "_" + want[0])
            out[name] = entry(*median_ms(lambda: fn(wt, sw, g1, gd, want=want, out=o, **kw), iters), cin, cout, h, w)
    return out


def torch_route(iters):
    import torch
    g = torch.Generator(device="cuda").manual_seed(2)
    h, w = DEC2
    (wt, sw), g1, gd = weights(g, 128, 64, 64), act(g, 64, h, w), act(g, 64, h, w)
    s5 = sw.view(64, 192, 1, 1, 1)
    h0, w0 = (h + 1) // 2, (w + 1) // 2

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def c16(p):                                              # and back: one layout copy (at the logical width)
        b, c, l, hh, ww = p.shape
        return p.reshape(b, c // 16, 16, l, hh, ww).permute(0, 3, 1, 4, 5, 2).contiguous()

    def fn():
        dX = torch.nn.grad.conv3d_input((B, 192, L, h, w), wt, planar(g1), padding=1) + \
            torch.nn.grad.conv3d_input((B, 192, L, h, w), s5, planar(gd))
        d0 = torch.ops.aten.upsample_nearest3d_backward(dX[:, :128].contiguous(), [L, h, w], [B, 128, L, h0, w0], None, None, None)
        return c16(d0), c16(dX[:, 128:])
    res = entry(*median_ms(fn, iters), 192, 64, h, w)
    res["concat_bytes"] = 192 * 4 * B * L * h * w
    return {"torch_dgrad_dec2": res}


def train_steps(iters):
    """One forward + backward of Dec2BlockThrough -> LastBlock -> PredHead on sources that require grad, next to the same
    step with Dec2Block on sources that do not, at the default frame size; the frozen trunk runs once, outside the timing."""
    import numpy as np
    import torch
    from v2ce_toolbox_amd import losses, synth
    from v2ce_toolbox_amd.dec2_block import Dec2Block, Dec2BlockThrough
    from v2ce_toolbox_amd.last_block import LastBlock
    from v2ce_toolbox_amd.pred_head import PredHead
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    fr = synth.synthetic_frames(L + 1, *FRAME, seed=3).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).cuda()
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    m = m.eval().cuda()
    gt = m(x).clone() * 0.9
    h1, s2, x1 = m.forward_dec2_sources(x)
    out = {}
    for name, cls, through in (("step_dec2_block", Dec2Block, False), ("step_dec2_block_through", Dec2BlockThrough, True)):
        dec2, block, head = cls.from_model(m), LastBlock.from_model(m), PredHead.from_model(m)
        srcs = []
        for t in (h1, s2):
            c = t.clone().requires_grad_(through)
            c.lw, c.c16 = t.lw, True
            if hasattr(t, "absmax"):
                c.absmax = t.absmax
            srcs.append(c)

        def step():
            for c in srcs:
                c.grad = None
            losses.calculate_loss(head(block(dec2(*srcs), x1)), gt)[0].backward()
        med, best = median_ms(step, max(iters // 2, 3))
        out[name] = {"ms": med, "ms_min": best}
    out["input_grads_in_a_step_ms"] = out["step_dec2_block_through"]["ms"] - out["step_dec2_block"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_step", action="store_true", help="kernels and torch's route only")
    a = ap.parse_args()
    from v2ce_toolbox_amd import hip
    result = {"dec2_shape": [B, L, *DEC2], "frame": list(FRAME), "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
    result.update(kernels(a.iters))
    result.update(torch_route(a.iters))
    if not a.no_step:
        result.update(train_steps(a.iters))
    ms = lambda k: result[k]["ms"]
    # the same flops: the new call's TFLOP/s over the old entry's is the old entry's time over the new call's
    result["flop_parity_dec2_over_dec3"] = ms("convup_dgrad_dec3") / ms("convupn_dgrad_dec2")
    result["convupn_ratio_to_convup_at_dec3"] = ms("convupn_dgrad_dec3") / ms("convup_dgrad_dec3")
    result["speedup_over_torch"] = ms("torch_dgrad_dec2") / ms("convupn_dgrad_dec2")
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
