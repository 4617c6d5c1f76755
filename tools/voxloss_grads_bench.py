"""Rate of the stage-1 loss gradient (v2ce_voxloss_grads, csrc/voxlossgrads.hip) on 64 pairs of 346x260 as
[4, 16, 20, 260, 346].

One call must read pred and gt and write grad (3 x 4 bytes x numel = 1.38 GB); with a sequence term on, the prepare
kernel reads pred and gt once more (2.30 GB in all, workspace traffic not counted).  The call is timed per
``synth.synthetic_voxels`` regime for all terms, for the reference's default list and for the elementwise part alone
(which launches no prepare kernel): HIP events around each call, median of --iters after --warmup.  "TBps" is those
algorithmic bytes over the call's time: a whole-call figure, not a kernel's share of peak.

The comparison is what a user runs today: ``torch.autograd.grad`` of the same weighted sum of the expressions of
``tools/voxlosses_bench.py::torch_terms`` (f32 device ops; only the terms of the list are evaluated, their values are
checked against ``torch_terms`` first), forward and backward timed together, and the forward alone so that the
backward's share can be read off.  The parent commit has no gradient, so there is nothing else to compare with.
Before anything is timed our gradient is compared with torch's.  ``torch_terms`` pools 'pt' along the last axis of a
transposed view; where that disagrees, the comparison (and a second timing, ``torch_autograd_contiguous_pt_ms``) uses the
same pools written as ``avg_pool3d((k, 1, 1))`` over the contiguous [N, 1, D, H, W] volumes, and the record says so.

The kernels' own times come from a separate run under ``rocprofv3 --kernel-trace --stats`` with ``--configs`` naming one
list; ``--kernel-stats CONFIG=CSV`` merges such a table into the record.  ``--resources`` adds the compiler's resource
summary of the kernels (hipcc -Rpass-analysis=kernel-resource-usage; needs no GPU).  Prints one JSON line (--out writes
it)."""
import argparse
import csv
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from voxlosses_bench import timed, torch_terms  # noqa: E402

from v2ce_toolbox_amd import hip, synth  # noqa: E402
from v2ce_toolbox_amd import losses as VL  # noqa: E402

ALL_LOSS = ("pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2")
# config -> (loss list, weights of torch_terms' values in the same total)
CONFIGS = {
    "all": (ALL_LOSS, {"pyramid": 1000.0, "pt": 1000.0, "ef": 0.5, "match": 0.5, "compensation": 1.0, "norml1": 1e-5,
                       "norml2": 1e-5}),
    "default": (VL.DEFAULT_LOSS, {"pyramid": 1000.0, "ef": 0.5, "compensation": 1.0}),
    "elementwise": (None, {"mse": 1.0}),
}
KERNELS = ("prepare_kernel", "comp_finish_kernel", "grad_kernel")


def coeffs(config, pred):
    loss, _ = CONFIGS[config]
    if loss is None:                                   # d mse / d pred alone
        c = hip.VoxLossGradCoeffs(struct_size=ctypes.sizeof(hip.VoxLossGradCoeffs))
        c.a_sq = 2.0 / pred.numel()
        return c
    sq = float(np.sum(VL.voxel_losses_batch(pred, pred, terms=()).pred_sq_sum)) if "norml2" in loss else None
    return VL.grad_coeffs(tuple(pred.shape), loss, pred_sq_sum=sq)


def term_fns(p, g, contiguous_pt=False):
    """The expressions of torch_terms, one callable per term, so that a list pays for its own terms only."""
    F = torch.nn.functional
    B, L, C, H, W = p.shape
    vol = lambda t: t.reshape(B, L, 2, 10, H, W).permute(0, 2, 1, 3, 4, 5).reshape(B * 2, L * 10, H, W)
    sp = lambda t: t.reshape(B, L, 2, 10, H, W)

    def pyramid():
        pv, gv = vol(p), vol(g)
        return sum(F.mse_loss(F.avg_pool3d(pv, k, k), F.avg_pool3d(gv, k, k)) for k in (2, 4, 8)) / 3

    def pt():
        if contiguous_pt:
            pv, gv = vol(p).unsqueeze(1), vol(g).unsqueeze(1)
            pool = lambda t, k, pad: F.avg_pool3d(t, (k, 1, 1), (k, 1, 1), (pad, 0, 0))
            return (F.mse_loss(pv, gv) + F.mse_loss(pool(pv, 3, 1), pool(gv, 3, 1)) +
                    F.mse_loss(pool(pv, 5, 0), pool(gv, 5, 0))) / 2
        a, b = (t.reshape(B * 2, L * 10, H * W).transpose(1, 2) for t in (vol(p), vol(g)))
        return (F.mse_loss(a, b) + F.mse_loss(F.avg_pool1d(a, 3, 3, 1), F.avg_pool1d(b, 3, 3, 1)) +
                F.mse_loss(F.avg_pool1d(a, 5, 5), F.avg_pool1d(b, 5, 5))) / 2

    def ef():
        ap_, ag = p.abs(), g.abs()
        e = 5 * F.mse_loss(ap_.sum(2), ag.sum(2)) + F.mse_loss(ap_.sum((1, 2)), ag.sum((1, 2)))
        es = 5 * F.mse_loss(sp(ap_).sum(3), sp(ag).sum(3)) + F.mse_loss(sp(ap_).sum((1, 3)), sp(ag).sum((1, 3)))
        return (e + 2 * es) / 2

    def compensation():
        mp, mg = p > 0.01, g > 0.01
        return F.mse_loss((p * mp).sum((2, 3)) / mp.sum((2, 3)).clamp(min=1), (g * mg).sum((2, 3)) / mg.sum((2, 3)).clamp(min=1))

    return {"mse": lambda: F.mse_loss(p, g), "pyramid": pyramid, "pt": pt, "ef": ef, "compensation": compensation,
            "match": lambda: F.nll_loss(torch.log(F.softmax(p, dim=1)), g.argmax(dim=1)),
            "norml1": lambda: torch.norm(p, p=1), "norml2": lambda: torch.norm(p, p=2)}


def torch_total(p, g, weights, contiguous_pt=False):
    t = term_fns(p, g, contiguous_pt)
    return sum(w * t[k]() for k, w in weights.items())


def resource_summary():
    """VGPRs, scratch, LDS and occupancy of every kernel of csrc/voxlossgrads.hip from the compiler's remarks."""
    src = os.path.join(hip.CSRC, "voxlossgrads.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), m.group(1))
            if "grad_kernel" in name:
                name += "<seq>" if "ILb1EE" in m.group(1) else "<volume>"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def kernel_stats(path):
    """Per kernel of this file: calls, average and minimum ns from a rocprofv3 --stats kernel table."""
    out = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in row["Name"]:
                key = k + ("<seq>" if "<true>" in row["Name"] else "<volume>" if "<false>" in row["Name"] else "")
                out[key] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                            "min_us": round(float(row["MinNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--regimes", nargs="*", default=["sparse", "frac", "stress"])
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.autograd comparison (profiling runs)")
    ap.add_argument("--resources", action="store_true", help="add the compiler's resource summary of the kernels")
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="CONFIG=CSV")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    H, W, B, Lq = 260, 346, a.B, a.L
    lib = hip.lib()
    st = hip.stream_ptr()
    size = ctypes.sizeof(hip.VoxLossGradCoeffs)
    rec = {"tool": "tools/voxloss_grads_bench.py", "device": torch.cuda.get_device_name(0), "shape": [B, Lq, 20, H, W],
           "regimes": {}}
    agree = True
    for regime in a.regimes:
        mk = lambda seed: torch.from_numpy(synth.synthetic_voxels(B * Lq, H, W, seed=seed, regime=regime)).cuda().reshape(
            B, Lq, 20, H, W)
        pred, gt = mk(1), mk(2)
        grad = torch.empty_like(pred)
        r = {}
        if not a.no_torch:
            with torch.no_grad():                       # the expressions timed below are torch_terms' own
                ref = torch_terms(pred, gt)
                mine = term_fns(pred, gt)
                for k, v in ref.items():                # (device reductions are not bit-reproducible run to run)
                    assert abs(float(mine[k]()) - float(v)) <= 1e-5 * abs(float(v)), k
                del ref, mine
        for config in a.configs:
            c = coeffs(config, pred)
            nb = lib.v2ce_voxloss_grads_workspace_bytes(B, Lq, 20, H, W, ctypes.byref(c), size)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            prepared = bool(any(c.a_ef) or c.a_comp or c.a_match)
            nbytes = (5 if prepared else 3) * 4 * pred.numel()

            def call():
                hip.check(lib.v2ce_voxloss_grads(pred.data_ptr(), gt.data_ptr(), B, Lq, 20, H, W, ctypes.byref(c), size, None,
                                                 grad.data_ptr(), ws.data_ptr(), nb, st), "v2ce_voxloss_grads")
            med, mn = timed(call, a.warmup, a.iters)
            q = {"ms": round(med, 4), "ms_min": round(mn, 4), "algorithmic_bytes": nbytes, "prepare_kernel_runs": prepared,
                 "TBps": round(nbytes / (med * 1e-3) / 1e12, 3), "workspace_bytes": int(nb)}
            if not a.no_torch:
                weights = CONFIGS[config][1]
                p = pred.clone().requires_grad_()

                def diff(contiguous_pt):
                    (theirs,) = torch.autograd.grad(torch_total(p, gt, weights, contiguous_pt), p)
                    return float((grad - theirs).abs().max()) / float(theirs.abs().max())
                q["max_abs_diff_to_torch_f32_over_max"] = diff(False)
                fix = "pt" in weights and q["max_abs_diff_to_torch_f32_over_max"] >= 1e-3
                if fix:
                    q["max_abs_diff_to_torch_f32_contiguous_pt_over_max"] = diff(True)
                    q["note"] = ("torch's gradient of 'pt' pooled along the last axis of a transposed view differs from ours; "
                                 "with the same pools over the contiguous volumes it agrees")
                q["agrees_with_torch_f32"] = (q["max_abs_diff_to_torch_f32_contiguous_pt_over_max"] if fix else
                                              q["max_abs_diff_to_torch_f32_over_max"]) < 1e-3
                agree = agree and q["agrees_with_torch_f32"]

                def torch_call(contiguous_pt=False):
                    (t,) = torch.autograd.grad(torch_total(p, gt, weights, contiguous_pt), p)
                    return t

                def torch_forward():
                    with torch.no_grad():
                        return torch_total(p, gt, weights)
                n_t = max(3, a.iters // 4)
                med_t, mn_t = timed(torch_call, 1, n_t)
                med_f, _ = timed(torch_forward, 1, n_t)
                q.update(torch_autograd_ms=round(med_t, 4), torch_autograd_ms_min=round(mn_t, 4),
                         torch_forward_only_ms=round(med_f, 4), torch_backward_share_ms=round(med_t - med_f, 4),
                         torch_autograd_over_ours=round(med_t / med, 2),
                         torch_backward_share_over_ours=round((med_t - med_f) / med, 2))
                if fix:
                    med_c, _ = timed(lambda: torch_call(True), 1, n_t)
                    q.update(torch_autograd_contiguous_pt_ms=round(med_c, 4),
                             torch_autograd_contiguous_pt_over_ours=round(med_c / med, 2))
                del p
            r[config] = q
            torch.cuda.empty_cache()
        rec["regimes"][regime] = r
        del pred, gt, grad
        torch.cuda.empty_cache()
    for item in a.kernel_stats:
        config, path = item.split("=", 1)
        rec.setdefault("kernel_us", {})[config] = kernel_stats(path)
    if a.resources:
        rec["compiler_resource_summary"] = resource_summary()
    rec.update({"iters": a.iters, "warmup": a.warmup, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                **hip.provenance()})
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    assert agree, "a gradient differs from torch's f32 autograd by more than 1e-3 of the largest element"


if __name__ == "__main__":
    main()
