"""Recipe of tests/golden/.voxmetrics/*.npz: inputs of the stage-1 score and the batched voxeliser with the REFERENCE's
own results on them.

The top level of tests/golden/ is the output set of oracle/make_goldens.py, so these fixtures sit in a directory of
their own.  The metric classes are loaded from the reference's train/scripts/model/metrics.py by path (it imports torch
and einops only); gen_discretized_event_volume and its two helpers are pulled out of train/scripts/utils/events_utils.py
with ast (the module imports h5py) and run under torch.set_num_threads(1), which is the serial put_.  Runs where the
reference tree is present; not collected by pytest.

    python tests/make_voxmetrics_goldens.py [out_dir]   (default tests/golden/.voxmetrics; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])


def reference_metrics():
    path = os.path.join(REF, "train", "scripts", "model", "metrics.py")
    spec = importlib.util.spec_from_file_location("ref_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_voxelizer():
    path = os.path.join(REF, "train", "scripts", "utils", "events_utils.py")
    tree = ast.parse(open(path).read(), path)
    want = {"calc_floor_ceil_delta", "create_update", "gen_discretized_event_volume"}
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == 3
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["gen_discretized_event_volume"]


def metric_cases():
    rng = np.random.default_rng(12)
    out = {}
    # b=2, l=3, h=11, w=13: sparse voxels around the threshold, a few exact zeros
    p = (rng.random((2, 3, 20, 11, 13), dtype=np.float32) * 0.03) * (rng.random((2, 3, 20, 11, 13)) < 0.6)
    g = (rng.random((2, 3, 20, 11, 13), dtype=np.float32) * 0.03) * (rng.random((2, 3, 20, 11, 13)) < 0.6)
    out["b2_l3_11x13"] = (p.astype(np.float32), g.astype(np.float32))
    # b=1, l=4, h=9, w=10: LDATI-like magnitudes, values at exactly f32(0.01)
    p = rng.exponential(0.05, (1, 4, 20, 9, 10)).astype(np.float32) * (rng.random((1, 4, 20, 9, 10)) < 0.3)
    g = rng.exponential(0.05, (1, 4, 20, 9, 10)).astype(np.float32) * (rng.random((1, 4, 20, 9, 10)) < 0.3)
    p.reshape(-1)[::17] = np.float32(0.01)
    g.reshape(-1)[::23] = np.float32(0.01)
    out["b1_l4_9x10"] = (p, g)
    # all-zero GT: F1 = 0
    p = rng.random((1, 2, 20, 8, 8), dtype=np.float32) * 0.05
    out["b1_l2_zero_gt"] = (p, np.zeros_like(p))
    return out


def metric_results(M, p, g):
    pt, gt = torch.from_numpy(p), torch.from_numpy(g)
    res = {}
    for op in ("raw", "sum_c", "sum_cp"):
        res[f"BinaryMatch_{op}"] = M.BinaryMatch(op_type=op)(pt, gt).numpy()
        res[f"BinaryMatchF1_{op}"] = M.BinaryMatchF1(op_type=op)(pt, gt).numpy()
    for k in (1, 2, 3, 4):
        if k <= min(10 * p.shape[1], p.shape[3], p.shape[4]):
            res[f"PoolMSE_{k}"] = M.PoolMSE(kernel_size=k)(pt, gt).numpy()
    res["MeanRatio"] = M.MeanRatio()(pt, gt).numpy()
    res["L1"] = torch.nn.L1Loss()(pt, gt).numpy()
    return res


def events(rng, n, H, W, pol, t1=33333):
    e = np.zeros(n, EVENT_DTYPE)
    e["timestamp"] = np.sort(rng.integers(0, t1, n)) if n else []
    e["x"], e["y"], e["polarity"] = rng.integers(0, W, n), rng.integers(0, H, n), rng.choice(pol, n)
    return e


def vox_cases():
    rng = np.random.default_rng(13)
    H, W = 7, 9
    return {
        "pm1_small": [events(rng, 400, H, W, [-1, 1]), events(rng, 1, H, W, [-1, 1]), events(rng, 900, H, W, [-1, 1])],
        "01_small": [events(rng, 700, H, W, [0, 1]), events(rng, 50, H, W, [0, 1])],
        "pm1_large": [events(rng, 40000, H, W, [-1, 1]), events(rng, 33000, 5, 6, [0, 1])],
    }


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(1)
    M = reference_metrics()
    for name, (p, g) in metric_cases().items():
        res = metric_results(M, p, g)
        path = os.path.join(out_dir, f"metrics_{name}.npz")
        np.savez_compressed(path, pred=p, gt=g, **{f"ref_{k}": v for k, v in res.items()})
        print(path, os.path.getsize(path))
    vox = reference_voxelizer()
    H, W, bins = 7, 9, 10
    for name, lists in vox_cases().items():
        ev = np.concatenate(lists)
        counts = np.array([len(e) for e in lists], np.int64)
        vols = []
        for e in lists:
            if len(e) < 2 or e["timestamp"].min() == e["timestamp"].max():
                vols.append(np.zeros((2 * bins, H, W), np.float32))
                continue
            vols.append(vox(e.copy(), (2 * bins, H, W)).numpy())
        path = os.path.join(out_dir, f"voxelize_{name}.npz")
        np.savez_compressed(path, events=ev, counts=counts, bins=np.int64(bins), H=np.int64(H), W=np.int64(W),
                            volume=np.stack(vols))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".voxmetrics"))
