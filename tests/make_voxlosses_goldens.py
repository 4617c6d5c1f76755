"""Recipe of tests/golden/.voxlosses/*.npz: voxel pairs with the REFERENCE's own stage-1 loss terms on them.

The loss classes are loaded from the reference's train/scripts/model/losses.py by path (it imports torch and einops
only); ``ModelInterface.calculate_loss`` is pulled out of train/scripts/model/model_interface.py with ast (the module
imports pytorch_lightning) and run with a stub ``self`` that carries hparams, the loss classes and ``ef_loss``.  Every
value is stored twice: ``ref_*`` from the f32 inputs, as the reference runs, and ``ref64_*`` from the same code on
``.double()`` inputs, which measures the reference's own rounding.  Runs where the reference tree is present; not
collected by pytest.

    python tests/make_voxlosses_goldens.py [out_dir]   (default tests/golden/.voxlosses; V2CE_REFERENCE_ROOT names the tree)
"""
import ast
import importlib.util
import logging
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
from einops import rearrange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxlosses_ref as R  # noqa: E402

EF_KEY = {"only_c": "only_c", "cl": "cl", "c+cl": "c_cl"}
ALL_LOSS = ["pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2"]
DEFAULT_LOSS = ["pyramid", "ef", "ef_splitp", "compensation"]
FULL = dict(L=16, H=260, W=346, pred_seed=1, gt_seed=2, regime="sparse")


def reference_losses():
    path = os.path.join(REF, "train", "scripts", "model", "losses.py")
    spec = importlib.util.spec_from_file_location("ref_losses", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_calculate_loss():
    path = os.path.join(REF, "train", "scripts", "model", "model_interface.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ModelInterface"]
    assert len(cls) == 1
    fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "calculate_loss"]
    assert len(fns) == 1
    ns = {"torch": torch, "rearrange": rearrange, "logger": logging.getLogger("ref")}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["calculate_loss"]


def run(M, calc, preds, gt, loss, ef_type="c+cl", add_base_loss=False, double=False):
    """The reference's (loss, loss_dict) as numpy scalars; preds: list of stages."""
    hp = SimpleNamespace(loss=list(loss), ef_type=ef_type, add_base_loss=add_base_loss, alpha_pyramid=1000, alpha_ef=0.5,
                         alpha_efc=5, alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5)
    stub = SimpleNamespace(hparams=hp, ef_loss=torch.nn.MSELoss(),
                           loss_function={"pyramid": M.Pyramid3dLoss(add_base_loss=add_base_loss),
                                          "pt": M.PyramidTemporalLoss(), "match": M.MatchLoss(),
                                          "compensation": M.CompensationLoss()})
    cast = (lambda a: torch.from_numpy(a).double()) if double else torch.from_numpy
    stages = [cast(p) for p in preds]
    total, d = calc(stub, {"voxels": cast(gt)}, {"voxels": stages if len(stages) > 1 else stages[0]})
    return total.numpy(), {k: v.numpy() for k, v in d.items()}


def results(M, calc, p, g, pyramid=True, p2=None):
    """ref_* / ref64_* of every term, ef_type and add_base_loss, and the default-list total."""
    out = {}
    every = [n for n in ALL_LOSS if pyramid or n != "pyramid"]
    default = [n for n in DEFAULT_LOSS if pyramid or n != "pyramid"]
    for double, pre in ((False, "ref_"), (True, "ref64_")):
        for ef_type, ek in EF_KEY.items():
            for base in (False, True):
                total, d = run(M, calc, [p], g, every, ef_type, base, double)
                out[f"{pre}ef_both_{ek}"] = d["ef_loss"]
                if pyramid:
                    out[f"{pre}pyramid_base{int(base)}"] = d["pyramid_loss"]
                out[f"{pre}loss_all_{ek}_base{int(base)}"] = total
            for kind in ("ef", "ef_splitp"):
                out[f"{pre}{kind}_only_{ek}"] = run(M, calc, [p], g, [kind], ef_type, False, double)[1]["ef_loss"]
        for k in ("pt_loss", "match", "compensation", "norml1", "norml2"):
            out[f"{pre}{k}"] = d[k]
        out[f"{pre}loss_default"] = run(M, calc, [p], g, default, double=double)[0]
        if p2 is not None:
            total, d = run(M, calc, [p, p2], g, every, double=double)
            out[f"{pre}stages_loss"] = total
            for k, v in d.items():
                out[f"{pre}stages_{k}"] = v
    return out


def sparse(rng, shape, scale, density):
    return (rng.exponential(scale, shape) * (rng.random(shape) < density)).astype(np.float32)


def cases():
    """name -> (pred, gt, second stage or None).  Magnitudes stay far below a spread of 80 along l (match_low == 0)."""
    rng = np.random.default_rng(131)
    out = {}
    out["b1_l1_8x8"] = (sparse(rng, (1, 1, 20, 8, 8), 0.5, 0.5), sparse(rng, (1, 1, 20, 8, 8), 0.5, 0.5), None)
    out["b1_l1_9x15"] = (sparse(rng, (1, 1, 20, 9, 15), 0.05, 0.4), sparse(rng, (1, 1, 20, 9, 15), 0.05, 0.4), None)
    s = (2, 3, 20, 11, 13)
    out["b2_l3_11x13"] = (sparse(rng, s, 2.0, 0.5), sparse(rng, s, 2.0, 0.5), sparse(rng, s, 1.0, 0.5))
    s = (1, 4, 20, 16, 24)
    out["b1_l4_16x24"] = (sparse(rng, s, 0.3, 0.3), sparse(rng, s, 0.3, 0.3), None)
    s = (3, 2, 20, 8, 70)
    out["b3_l2_8x70"] = (sparse(rng, s, 0.1, 0.25), sparse(rng, s, 0.1, 0.25), None)
    s = (1, 3, 20, 8, 10)
    out["zero_gt"] = (sparse(rng, s, 0.2, 0.6), np.zeros(s, np.float32), None)
    s = (1, 2, 20, 9, 12)
    p, g = sparse(rng, s, 0.02, 0.5), sparse(rng, s, 0.02, 0.5)
    thr = np.float32(0.01)
    above = np.nextafter(thr, np.float32(1))
    p.reshape(-1)[::7] = thr
    p.reshape(-1)[3::11] = above
    g.reshape(-1)[::5] = thr
    g.reshape(-1)[2::13] = above
    out["at_threshold"] = (p, g, None)
    return out


def full_inputs(cfg=FULL):
    from v2ce_toolbox_amd import synth
    mk = lambda seed: synth.synthetic_voxels(cfg["L"], cfg["H"], cfg["W"], seed=seed, regime=cfg["regime"]).reshape(
        1, cfg["L"], 20, cfg["H"], cfg["W"])
    return mk(cfg["pred_seed"]), mk(cfg["gt_seed"])


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    M, calc = reference_losses(), reference_calculate_loss()
    for name, (p, g, p2) in cases().items():
        assert all(s["match_low"] == 0 for s in R.batch_stats(p, g)), name
        extra = {} if p2 is None else {"pred2": p2}
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, pred=p, gt=g, **extra, **results(M, calc, p, g, p2=p2))
        print(path, os.path.getsize(path))
    p, g = full_inputs()
    assert R.seq_stats(p[0], g[0], terms=("match",))["match_low"] == 0
    path = os.path.join(out_dir, "full_b1_l16_260x346.npz")
    np.savez_compressed(path, **{k: np.array(v) for k, v in FULL.items()}, pred_sum=p.astype(np.float64).sum(),
                        gt_sum=g.astype(np.float64).sum(), **results(M, calc, p, g))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".voxlosses"))
