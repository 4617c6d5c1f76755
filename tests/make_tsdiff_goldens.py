"""Recipe of tests/golden/.tsdiff/tsdiff_g11_*.npz: inputs of the stage-2 score and the REFERENCE's own result on them.

The top level of tests/golden/ is exactly the output set of oracle/make_goldens.py (test_oracle_goldens_recipe compares
the two file for file), so these fixtures of a second recipe sit in a directory of their own that it skips.

ts_diff_metric is pulled out of the reference's train/scripts/stage2/stage2_metrics.py with ast and executed with
``np`` and a ``logger`` supplied (importing the module needs h5py and pathlib2, and its logger exists only under
__main__).  Runs where the reference tree is present; not collected by pytest.

    python tests/make_tsdiff_goldens.py [out_dir]      (default tests/golden/.tsdiff; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
EVENT_DTYPE = np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")])


def reference_ts_diff_metric():
    path = os.path.join(REF, "train", "scripts", "stage2", "stage2_metrics.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "ts_diff_metric"]
    assert len(fn) == 1
    ns = {"np": np, "logger": logging.getLogger("tsdiff_goldens")}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["ts_diff_metric"]


def events(ts, x, y, p):
    e = np.zeros(len(ts), EVENT_DTYPE)
    e["timestamp"], e["x"], e["y"], e["polarity"] = ts, x, y, p
    return e


def cases():
    out = {}
    rng = np.random.default_rng(11)

    def rand(n, x0, x1, y0, y1, pol, t1=33333):
        return events(rng.integers(0, t1, n), rng.integers(x0, x1, n), rng.integers(y0, y1, n), rng.choice(pol, n))

    out["r0_fps30_pm1"] = (rand(1500, 100, 140, 50, 80, [-1, 1]), rand(5000, 100, 140, 50, 80, [0, 1]), 0, 30.0)
    out["r1_fps31.7_01"] = (rand(1500, 100, 140, 50, 80, [0, 1]), rand(3000, 100, 140, 50, 80, [0, 1]), 1, 31.7)
    out["r3_fps10_pm1"] = (rand(800, 0, 346, 0, 260, [-1, 1]), rand(6000, 0, 346, 0, 260, [0, 1]), 3, 10.0)
    out["empty_pred"] = (rand(500, 0, 346, 0, 260, [-1, 1]), rand(0, 0, 346, 0, 260, [0, 1]), 1, 30.0)
    bx = np.array([0, 1, 344, 345]); by = np.array([0, 1, 258, 259])
    g = events(rng.integers(0, 33333, 1200), rng.choice(bx, 1200), rng.choice(by, 1200), rng.choice([-1, 1], 1200))
    pr = events(rng.integers(0, 33333, 3000), rng.choice(bx, 3000), rng.choice(by, 3000), rng.choice([0, 1], 3000))
    out["borders_r3"] = (g, pr, 3, 30.0)
    g = events(rng.integers(0, 33333, 1000), rng.integers(199, 202, 1000), rng.integers(99, 102, 1000), rng.choice([0, 1], 1000))
    pr = events(rng.integers(0, 3000, 6000) * 11, np.full(6000, 200), np.full(6000, 100), rng.choice([0, 1], 6000))
    out["dense_cell_r1"] = (g, pr, 1, 30.0)
    return out


def main(out_dir):
    f = reference_ts_diff_metric()
    os.makedirs(out_dir, exist_ok=True)
    for name, (gt, pred, r, fps) in cases().items():
        res = np.asarray(f(gt.copy(), pred.copy(), search_range=r, fps=fps), dtype=np.float64)
        path = os.path.join(out_dir, f"tsdiff_g11_{name}.npz")
        np.savez_compressed(path, gt=gt, pred=pred, search_range=np.int64(r), fps=np.float64(fps), result=res)
        print(path, res, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".tsdiff"))
