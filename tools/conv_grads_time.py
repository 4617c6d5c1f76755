"""Time the gradient kernels of the trainable decoder chain (conv_grads.py) at the shapes of their layers, torch's own
route for the same gradients, and one optimizer step of the ``finetune.fit_*``.  Prints one JSON line.

    python tools/conv_grads_time.py [--rows NAME ...] [--iters 10] [--no_fit] [--no_torch] [--out profiles/NAME.json]
                                    [--fits fit_dec1_conv ...] [--fit_shape L H W]
                                    [--parent_lib libv2ce_hip_parent.so [--rounds 2]]

``ROWS`` is the table: a name, the checked entry pair of ``conv_grads`` (``<entry>_wgrad`` / ``<entry>_dgrad``), the channel
counts and [B, L, H, W].  A row of one channel count c is a 3x3x3 convolution c -> c behind a relu (the conv2 layers: x, y,
upstream -> weight and shift; weight, y, upstream -> x and res); a row of three, (c0, c1, cout), is conv1 and the 1x1x1
shortcut on cat(upsample(x0), x1) (x0, x1, g1, gd -> weight, short, short_bias; weight, short, g1, gd -> x0 and x1).  Every
row is timed with all outputs and with the outputs the training layers ask for alone.  The default rows are the layers of
``UNet.decoders[3]``, ``[2]`` and ``[1].conv2`` at the default frame size, the wider 3x3x3 shapes of ``decoders[0]`` and the
resblocks, and the 32-channel entries at the 64-channel ones' shapes (the same kernel templates at equal flops or positions).

Kernel times are medians (and minima) of HIP-event intervals after three warm-up calls; TFLOP/s counts 2 * cout * cin * 27
* positions (28 with the shortcut) against the 155 TF peak of the exact-f32 MFMA.  ``torch_*``: conv3d weight / input
gradients on planar f32 (MIOpen) with the layout copies a channels-last-16 caller pays, for the rows of ``TORCH_ROWS``.
``fit_*_step``: wall time per step from two fits of different lengths, so that the cached pass of the frozen trunk cancels.

--parent_lib: a build of another commit's library in v2ce-toolbox_amd/csrc, next to this tree's as in tools/lib_ab.sh.  The
3x3x3 rows whose entries that library has are then timed through the C ABI in fresh processes of their own in the order
parent, new, parent, new, ... and recorded under "ab": per entry each library's rounds and the ratio of their medians."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
FRAME, DEC2, DEC1 = (1, 16, 260, 346), (1, 16, 130, 173), (1, 16, 65, 87)
ROWS = (
    ("conv32_dec3", "conv32", (32,), FRAME),                 # decoders[3].conv2
    ("conv32_dec3_b4", "conv32", (32,), (4,) + FRAME[1:]),
    ("convup_dec3", "convup", (64, 32, 32), FRAME),          # decoders[3].conv1 and shortcut
    ("convn_64", "convn", (64,), DEC2),                      # decoders[2].conv2
    ("conv32", "conv32", (32,), DEC2),                       # the 32-channel entries at the same positions
    ("convupn_dec2", "convupn", (128, 64, 64), DEC2),        # decoders[2].conv1 and shortcut
    ("convupn_dec3", "convupn", (64, 32, 32), FRAME),        # the N-channel entries at the last block's shape
    ("convc_128", "convc", (128,), DEC1),                    # decoders[1].conv2
    ("convc_256", "convc", (256,), (1, 16, 33, 44)),         # the shape of decoders[0].conv2
    ("convc_512", "convc", (512,), (1, 16, 17, 22)),         # the shape of the resblocks
)
TORCH_ROWS = ("conv32_dec3", "convup_dec3", "convn_64", "convupn_dec2", "convc_128")
FITS = ("fit_head", "fit_tail", "fit_tail_norms", "fit_last_block", "fit_dec2_conv", "fit_dec2_block", "fit_dec1_conv")


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


def act(g, c, shape):
    """A channels-last-16 activation [B, L, c / 16, H, pitch, 16] of logical width W."""
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    B, L, H, W = shape
    t = torch.randn((B, L, c // 16, H, V2ce3d._pitch(W), 16), generator=g, device="cuda")
    t.lw, t.c16 = W, True
    return t


def half(shape):
    return shape[:2] + ((shape[2] + 1) // 2, (shape[3] + 1) // 2)


def entry(med, best, cin, cout, units, shape):
    flop = 2.0 * cout * cin * units * shape[0] * shape[1] * shape[2] * shape[3]
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF,
            "gflop": flop / 1e9, "shape": list(shape)}


def conv2_tensors(g, c, shape):
    import torch
    return act(g, c, shape), act(g, c, shape), act(g, c, shape), 0.05 * torch.randn((c, c, 3, 3, 3), generator=g, device="cuda")


def conv1_tensors(g, chans, shape):
    import torch
    c0, c1, cout = chans
    return (act(g, c0, half(shape)), act(g, c1, shape), act(g, cout, shape), act(g, cout, shape),
            0.05 * torch.randn((cout, c0 + c1, 3, 3, 3), generator=g, device="cuda"),
            0.1 * torch.randn((cout, c0 + c1), generator=g, device="cuda"))


def time_row(name, prefix, chans, shape, iters, g):
    import torch
    from v2ce_toolbox_amd import conv_grads
    wg, dg = getattr(conv_grads, prefix + "_wgrad"), getattr(conv_grads, prefix + "_dgrad")
    if len(chans) == 1:
        c = chans[0]
        x, y, up, w = conv2_tensors(g, c, shape)
        ow = {"weight": torch.empty_like(w), "shift": torch.empty(c, device="cuda")}
        ox = {"x": torch.empty_like(up), "res": torch.empty_like(up)}
        return {name + "_wgrad": entry(*median_ms(lambda: wg(x, y, up, out=ow), iters), c, c, 27, shape),
                name + "_dgrad": entry(*median_ms(lambda: dg(w, y, up, out=ox), iters), c, c, 27, shape),
                name + "_dgrad_x_alone": entry(*median_ms(lambda: dg(w, y, up, want=("x",), out={"x": ox["x"]}), iters),
                                               c, c, 27, shape)}
    c0, c1, cout = chans
    x0, x1, g1, gd, w, sw = conv1_tensors(g, chans, shape)
    ow = {"weight": torch.empty_like(w), "short": torch.empty_like(sw), "short_bias": torch.empty(cout, device="cuda")}
    ox = {"x0": torch.empty_like(x0), "x1": torch.empty_like(x1)}
    out = {name + "_wgrad": entry(*median_ms(lambda: wg(x0, x1, g1, gd, out=ow), iters), c0 + c1, cout, 28, shape),
           name + "_wgrad_weight_alone": entry(*median_ms(lambda: wg(x0, x1, g1, gd, want=("weight",), out={"weight": ow["weight"]}),
                                                          iters), c0 + c1, cout, 27, shape),
           name + "_dgrad": entry(*median_ms(lambda: dg(w, sw, g1, gd, out=ox), iters), c0 + c1, cout, 28, shape)}
    for n, cin in (("x0", c0), ("x1", c1)):
        kw = {"c0": c0} if prefix == "convupn" and n == "x1" else {}       # (without x0 the entry cannot tell c0 from c1)
        out[f"{name}_dgrad_{n}"] = entry(*median_ms(lambda: dg(w, sw, g1, gd, want=(n,), out={n: ox[n]}, **kw), iters),
                                         cin, cout, 28, shape)
    return out


def planar(t):
    """channels-last-16 -> torch's [B, C, L, H, W]: one layout copy."""
    p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
    return p[..., :t.lw].contiguous()


def c16(p):
    """and back: one layout copy (at the logical width)."""
    b, ch, l, h, w = p.shape
    return p.reshape(b, ch // 16, 16, l, h, w).permute(0, 3, 1, 4, 5, 2).contiguous()


def torch_row(name, chans, shape, iters, g):
    """torch's route for the row's two gradients, from and to channels-last-16; for a 3x3x3 row also on tensors that are
    channels-first already."""
    import torch
    import torch.nn.functional as F
    B, L, H, W = shape
    if len(chans) == 1:
        c = chans[0]
        x, y, up, w = conv2_tensors(g, c, shape)
        px, py, pu = planar(x), planar(y), planar(up)

        def masked(copies):
            return torch.where((planar(y) if copies else py) > 0, planar(up) if copies else pu, torch.zeros((), device="cuda"))

        def wgrad(copies=True):
            m = masked(copies)
            return torch.nn.grad.conv3d_weight(planar(x) if copies else px, w.shape, m, padding=1), m.sum(dim=(0, 2, 3, 4))

        def dgrad(copies=True):
            m = masked(copies)
            d = torch.nn.grad.conv3d_input((B, c, L, H, W), w, m, padding=1)
            return (c16(d), c16(m)) if copies else (d, m)
        return {f"torch_{name}_wgrad": entry(*median_ms(wgrad, iters), c, c, 27, shape),
                f"torch_{name}_dgrad": entry(*median_ms(dgrad, iters), c, c, 27, shape),
                f"torch_{name}_wgrad_channels_first": entry(*median_ms(lambda: wgrad(False), iters), c, c, 27, shape),
                f"torch_{name}_dgrad_channels_first": entry(*median_ms(lambda: dgrad(False), iters), c, c, 27, shape)}
    c0, c1, cout = chans
    x0, x1, g1, gd, w, sw = conv1_tensors(g, chans, shape)
    s5 = sw.view(cout, c0 + c1, 1, 1, 1)
    H0, W0 = half(shape)[2:]

    def wgrad():
        X = torch.cat([F.interpolate(planar(x0), size=(L, H, W), mode="nearest"), planar(x1)], dim=1)
        s = planar(gd)
        return (torch.nn.grad.conv3d_weight(X, w.shape, planar(g1), padding=1), torch.nn.grad.conv3d_weight(X, s5.shape, s),
                s.sum(dim=(0, 2, 3, 4)))

    def dgrad():
        dX = torch.nn.grad.conv3d_input((B, c0 + c1, L, H, W), w, planar(g1), padding=1) + \
            torch.nn.grad.conv3d_input((B, c0 + c1, L, H, W), s5, planar(gd))
        d0 = torch.ops.aten.upsample_nearest3d_backward(dX[:, :c0].contiguous(), [L, H, W], [B, c0, L, H0, W0], None, None, None)
        return c16(d0), c16(dX[:, c0:])
    return {f"torch_{name}_wgrad": entry(*median_ms(wgrad, iters), c0 + c1, cout, 28, shape),
            f"torch_{name}_dgrad": entry(*median_ms(dgrad, iters), c0 + c1, cout, 28, shape)}


def fit_steps(names, shape, iters):
    """One optimizer step of each fit with all its groups (SGD at 1e-6, inputs cached) on x [1, L, 2, H, W]: wall time per
    step from two fits of different lengths (the cached forward of the frozen trunk cancels)."""
    import numpy as np
    import torch
    from v2ce_toolbox_amd import finetune, synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    L, H, W = shape
    fr = synth.synthetic_frames(L + 1, H, W, seed=3).astype(np.float32) / 255
    x = torch.from_numpy(((np.stack([fr[:-1], fr[1:]], axis=1) - np.float32(0.153)) / np.float32(0.165))[None]).cuda()
    out = {}
    for name in names:
        fit = getattr(finetune, name)

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
        out[name + "_step"] = {"ms": (b - a) / (many - few) * 1e3, "steps_timed": many - few, "x": [1, L, 2, H, W]}
    return out


def raw_rows(lib_path, rows, iters):
    """The 3x3x3 rows through the C ABI of the library at `lib_path`, bound here: another commit's library may lack entries
    that ``hip.lib()`` binds.  Both sides of the A/B go through this function; a row whose entry is missing is left out."""
    import ctypes

    import torch
    lib = ctypes.CDLL(lib_path)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    g = torch.Generator(device="cuda").manual_seed(1)
    stream = torch.cuda.current_stream().cuda_stream or None
    out = {}
    for name, prefix, chans, shape in rows:
        if len(chans) != 1 or not hasattr(lib, f"v2ce_{prefix}_wgrad"):
            continue
        c = chans[0]
        x, y, up, w = conv2_tensors(g, c, shape)
        dims = (() if prefix == "conv32" else (c, c)) + tuple(shape) + (int(x.shape[4]),)
        for kind, first, outs in (("wgrad", x, (torch.empty_like(w), torch.empty(c, device="cuda"))),
                                  ("dgrad", w, (torch.empty_like(up), torch.empty_like(up)))):
            q, f = getattr(lib, f"v2ce_{prefix}_{kind}_workspace_bytes"), getattr(lib, f"v2ce_{prefix}_{kind}")
            q.argtypes, q.restype = [i32] * (len(dims) + 1), sz
            f.argtypes, f.restype = [vp] * 3 + [i32] * len(dims) + [vp, vp, vp, sz, i32, vp], i32
            nb = q(*dims, 0)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

            def call(f=f, first=first, outs=outs, ws=ws, nb=nb):
                rc = f(first.data_ptr(), y.data_ptr(), up.data_ptr(), *dims, outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr(),
                       nb, 0, stream)
                assert rc == 0, (prefix, kind, rc)
            out[f"{name}_{kind}"] = entry(*median_ms(call, iters), c, c, 27, shape)
    return out


def ab(parent_lib, names, rounds, iters):
    """The 3x3x3 rows under the parent's library and under this one, a fresh process each, parent first."""
    runs = {"parent": [], "new": []}
    for _ in range(rounds):
        for which, lib in (("parent", parent_lib), ("new", "libv2ce_hip.so")):
            path = os.path.join(ROOT, "v2ce-toolbox_amd", "csrc", lib)
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--raw_only", path, "--iters", str(iters), "--rows", *names],
                                  check=True, capture_output=True, text=True, timeout=240).stdout.strip().splitlines()[-1]
            runs[which].append(json.loads(line))
    med = lambda vs: sorted(vs)[len(vs) // 2]
    out = {"order": "parent, new" + ", parent, new" * (rounds - 1), "parent_lib": parent_lib}
    for k in runs["parent"][0]:
        p, n = [r[k]["ms"] for r in runs["parent"]], [r[k]["ms"] for r in runs["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_over_parent": med(n) / med(p)}
    out["worst_new_over_parent"] = max(v["new_over_parent"] for v in out.values() if isinstance(v, dict))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=None, metavar="NAME", help=f"of {[r[0] for r in ROWS]} (default: all)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no_fit", action="store_true", help="no step timings")
    ap.add_argument("--no_torch", action="store_true", help="no torch route")
    ap.add_argument("--fits", nargs="*", default=list(FITS), metavar="FIT", help="the fits whose step is timed (default: all seven)")
    ap.add_argument("--fit_shape", nargs=3, type=int, default=[FRAME[1], FRAME[2], FRAME[3]], metavar=("L", "H", "W"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_lib", default=None, help="file name of the parent commit's library in v2ce-toolbox_amd/csrc")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--raw_only", default=None, metavar="LIB",
                    help="the 3x3x3 rows through the C ABI of the library at this path, one JSON line (the A/B's child)")
    a = ap.parse_args()
    unknown = [n for n in a.rows or () if n not in [r[0] for r in ROWS]]
    if unknown:
        ap.error(f"unknown rows {unknown}")
    rows = [r for r in ROWS if a.rows is None or r[0] in a.rows]
    if a.raw_only:
        print(json.dumps(raw_rows(a.raw_only, rows, a.iters)))
        return 0
    import torch
    from v2ce_toolbox_amd import hip
    result = {"what": "tools/conv_grads_time.py", "rows": [r[0] for r in rows], "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
    g = torch.Generator(device="cuda").manual_seed(1)
    for row in rows:
        result.update(time_row(*row, a.iters, g))
    if not a.no_torch:
        for name, _, chans, shape in rows:
            if name in TORCH_ROWS:
                result.update(torch_row(name, chans, shape, a.iters, g))
                for kind in ("wgrad", "dgrad"):
                    result[f"{name}_{kind}_speedup_over_torch"] = result[f"torch_{name}_{kind}"]["ms"] / result[f"{name}_{kind}"]["ms"]
    if not a.no_fit:
        result.update(fit_steps(a.fits, a.fit_shape, a.iters))
    if a.parent_lib:
        result["ab"] = ab(a.parent_lib, [r[0] for r in rows], a.rounds, a.iters)
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
