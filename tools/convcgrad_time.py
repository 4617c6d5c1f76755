"""Time the gradient kernels of the wide 3x3x3 convolutions (v2ce_convc_wgrad, v2ce_convc_dgrad) at the shape of
UNet.decoders[1].conv2, [1, 16, 65, 87] at 128 -> 128; in the same run the 64-channel entries (v2ce_convn_wgrad,
v2ce_convn_dgrad) at 64 -> 64 on [1, 16, 130, 173], which has nearly the same flops, and torch's own route on channels-first
f32 at decoders[1]'s shape (conv3d weight / input gradients, MIOpen, plus the layout copies a channels-last-16 caller pays).
Also 256 -> 256 at [1, 16, 33, 44] and 512 -> 512 at [1, 16, 17, 22], the shapes of decoders[0].conv2 and of the resblocks.
Prints one JSON line.

    python tools/convcgrad_time.py [--iters 10] [--out profiles/NAME.json] [--parent_lib libv2ce_hip_parent.so [--rounds 2]]

Kernel times are medians of HIP-event intervals after three warm-up calls; TFLOP/s counts 2 * cout * cin * 27 * positions per
gradient against the 155 TF peak of the exact-f32 MFMA.

--parent_lib: a build of the parent commit's library in v2ce-toolbox_amd/csrc, next to this tree's as in tools/lib_ab.sh.  The
entries that existed before -- v2ce_convn_* at 64 -> 64 and v2ce_conv32_* on [1, 16, 130, 173] -- are then timed through the
C ABI in fresh processes of their own in the order parent, new, parent, new, ... and both libraries' times are recorded
under "ab": per entry each library's rounds and the ratio of their medians, new / parent."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 155.0
DEC1 = (1, 16, 65, 87)
DEC2 = (1, 16, 130, 173)
WIDER = ((256, (1, 16, 33, 44)), (512, (1, 16, 17, 22)))


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
    import torch
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    B, L, H, W = shape
    t = torch.randn((B, L, c // 16, H, V2ce3d._pitch(W), 16), generator=g, device="cuda")
    t.lw, t.c16 = W, True
    return t


def entry(med, best, c, shape):
    flop = 2.0 * c * c * 27 * shape[0] * shape[1] * shape[2] * shape[3]
    return {"ms": med, "ms_min": best, "tflops": flop / med / 1e9, "of_f32_mfma_peak": flop / med / 1e9 / PEAK_TF,
            "gflop": flop / 1e9, "shape": list(shape)}


def time_pair(wg, dg, c, shape, iters, g, tag):
    import torch
    x, y, up = act(g, c, shape), act(g, c, shape), act(g, c, shape)
    w = 0.05 * torch.randn((c, c, 3, 3, 3), generator=g, device="cuda")
    ow = {"weight": torch.empty_like(w), "shift": torch.empty(c, device="cuda")}
    ox = {"x": torch.empty_like(up), "res": torch.empty_like(up)}
    return {tag + "_wgrad": entry(*median_ms(lambda: wg(x, y, up, out=ow), iters), c, shape),
            tag + "_dgrad": entry(*median_ms(lambda: dg(w, y, up, out=ox), iters), c, shape),
            tag + "_dgrad_x_alone": entry(*median_ms(lambda: dg(w, y, up, want=("x",), out={"x": ox["x"]}), iters), c, shape)}


def older(iters):
    """The entries that existed before the wide ones: 64 -> 64 and 32 -> 32 at decoders[2]'s shape."""
    import torch
    from v2ce_toolbox_amd import conv_grads
    g = torch.Generator(device="cuda").manual_seed(1)
    out = time_pair(conv_grads.convn_wgrad, conv_grads.convn_dgrad, 64, DEC2, iters, g, "convn_64")
    out.update(time_pair(conv_grads.conv32_wgrad, conv_grads.conv32_dgrad, 32, DEC2, iters, g, "conv32"))
    return out


def older_raw(lib_path, iters):
    """The same four entries through the C ABI of the library at `lib_path`, bound here: a library of the parent commit has
    no v2ce_convc_* for ``hip.lib()`` to bind.  Both sides of the A/B go through this function."""
    import ctypes

    import torch
    L = ctypes.CDLL(lib_path)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    g = torch.Generator(device="cuda").manual_seed(1)
    B, Lq, H, W = DEC2
    stream = torch.cuda.current_stream().cuda_stream or None
    out = {}
    for c, sym, tag in ((64, "v2ce_convn_", "convn_64"), (32, "v2ce_conv32_", "conv32")):
        x, y, up = act(g, c, DEC2), act(g, c, DEC2), act(g, c, DEC2)
        w = 0.05 * torch.randn((c, c, 3, 3, 3), generator=g, device="cuda")
        dims = ((c, c) if c == 64 else ()) + (B, Lq, H, W, int(x.shape[4]))
        for kind, first, outs in (("wgrad", x, (torch.empty_like(w), torch.empty(c, device="cuda"))),
                                  ("dgrad", w, (torch.empty_like(up), torch.empty_like(up)))):
            q, f = getattr(L, sym + kind + "_workspace_bytes"), getattr(L, sym + kind)
            q.argtypes, q.restype = [i32] * (len(dims) + 1), sz
            f.argtypes, f.restype = [vp] * 3 + [i32] * len(dims) + [vp, vp, vp, sz, i32, vp], i32
            nb = q(*dims, 0)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

            def call(f=f, first=first, outs=outs, ws=ws, nb=nb):
                rc = f(first.data_ptr(), y.data_ptr(), up.data_ptr(), *dims, outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr(),
                       nb, 0, stream)
                assert rc == 0, (sym + kind, rc)
            out[f"{tag}_{kind}"] = entry(*median_ms(call, iters), c, DEC2)
    return out


def wide(iters):
    import torch
    from v2ce_toolbox_amd import conv_grads
    g = torch.Generator(device="cuda").manual_seed(3)
    out = time_pair(conv_grads.convc_wgrad, conv_grads.convc_dgrad, 128, DEC1, iters, g, "convc_128")
    for c, shape in WIDER:
        out.update(time_pair(conv_grads.convc_wgrad, conv_grads.convc_dgrad, c, shape, iters, g, f"convc_{c}"))
    return out


def torch_route(iters):
    import torch
    B, L, H, W = DEC1
    c = 128
    g = torch.Generator(device="cuda").manual_seed(2)
    x, y, up = act(g, c, DEC1), act(g, c, DEC1), act(g, c, DEC1)
    w = 0.05 * torch.randn((c, c, 3, 3, 3), generator=g, device="cuda")

    def planar(t):                                           # channels-last-16 -> torch's [B, C, L, H, W]: one layout copy
        p = t.permute(0, 2, 5, 1, 3, 4).reshape(t.shape[0], t.shape[2] * 16, t.shape[1], t.shape[3], t.shape[4])
        return p[..., :t.lw].contiguous()

    def c16(p):                                              # and back: one layout copy (at the logical width)
        b, ch, l, h, w_ = p.shape
        return p.reshape(b, ch // 16, 16, l, h, w_).permute(0, 3, 1, 4, 5, 2).contiguous()

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
    return {"torch_128_wgrad": entry(*median_ms(wgrad, iters), c, DEC1), "torch_128_dgrad": entry(*median_ms(dgrad, iters), c, DEC1),
            "torch_128_wgrad_channels_first": entry(*median_ms(lambda: wgrad(False), iters), c, DEC1),
            "torch_128_dgrad_channels_first": entry(*median_ms(lambda: dgrad(False), iters), c, DEC1)}


def ab(parent_lib, rounds, iters):
    """The older entries under the parent's library and under this one, a fresh process each, parent first."""
    runs = {"parent": [], "new": []}
    for _ in range(rounds):
        for which, lib in (("parent", parent_lib), ("new", None)):
            path = os.path.join(ROOT, "v2ce-toolbox_amd", "csrc", lib or "libv2ce_hip.so")
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--older_only", path, "--iters", str(iters)],
                                  check=True, capture_output=True, text=True, timeout=240).stdout.strip().splitlines()[-1]
            runs[which].append(json.loads(line))
    med = lambda vs: sorted(vs)[len(vs) // 2]
    out = {"order": "parent, new" + ", parent, new" * (rounds - 1), "parent_lib": parent_lib}
    for k in runs["new"][0]:
        p, n = [r[k]["ms"] for r in runs["parent"]], [r[k]["ms"] for r in runs["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_over_parent": med(n) / med(p)}
    out["worst_new_over_parent"] = max(v["new_over_parent"] for v in out.values() if isinstance(v, dict))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_lib", default=None, help="file name of the parent commit's library in v2ce-toolbox_amd/csrc")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--older_only", default=None, metavar="LIB",
                    help="the entries that existed before, through the C ABI of the library at this path, one JSON line (the A/B's child)")
    a = ap.parse_args()
    if a.older_only:
        print(json.dumps(older_raw(a.older_only, a.iters)))
        return 0
    from v2ce_toolbox_amd import hip
    result = {"what": "tools/convcgrad_time.py", "peak_tf": PEAK_TF, "iters": a.iters, **hip.provenance()}
    result.update(older(a.iters))
    result.update(wide(a.iters))
    result.update(torch_route(a.iters))
    ms = lambda k: result[k]["ms"]
    for kind in ("wgrad", "dgrad"):
        # per flop: 128 -> 128 on decoders[1]'s positions against 64 -> 64 on decoders[2]'s
        result[f"{kind}_128_time_per_flop_over_convn_64"] = (ms(f"convc_128_{kind}") / result[f"convc_128_{kind}"]["gflop"]) / \
            (ms(f"convn_64_{kind}") / result[f"convn_64_{kind}"]["gflop"])
        result[f"{kind}_128_speedup_over_torch"] = ms(f"torch_128_{kind}") / ms(f"convc_128_{kind}")
        result[f"{kind}_128_speedup_over_torch_channels_first"] = ms(f"torch_128_{kind}_channels_first") / ms(f"convc_128_{kind}")
    if a.parent_lib:
        result["ab"] = ab(a.parent_lib, a.rounds, a.iters)
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
