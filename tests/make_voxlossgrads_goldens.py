"""Recipe of tests/golden/.voxlossgrads/*.npz: voxel pairs with the REFERENCE's own autograd gradient of its stage-1 loss.

The reference's loss classes and ``ModelInterface.calculate_loss`` are loaded as tests/make_voxlosses_goldens.py loads
them; the prediction requires grad and ``total.backward()`` runs.  Stored per file: the inputs as f32, per config
``ref64_grad_<config>`` -- the gradient of the same code on ``.double()`` inputs, f64 -- and the scalar
``ref32_dev_<config>`` = max |grad32 - grad64| of the f32 run, which measures the reference's own rounding.  A config
with two refinement stages also stores ``ref64_grad_<config>_p2`` / ``ref32_dev_<config>_p2`` for the second stage.
Runs where the reference tree is present; not collected by pytest.

    python tests/make_voxlossgrads_goldens.py [out_dir]   (default tests/golden/.voxlossgrads)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxlosses_ref as R  # noqa: E402

ALL_LOSS = ("pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2")
DEFAULT_LOSS = ("pyramid", "ef", "ef_splitp", "compensation")
SIZE_CAP = 300_000
# config -> the keyword arguments of calculate_loss; `staged` configs run on [pred, pred2]
CONFIGS = {name: dict(loss=(name,)) for name in ALL_LOSS}
CONFIGS.update({
    "default": dict(loss=DEFAULT_LOSS),
    "full_c_cl_base1": dict(loss=ALL_LOSS, ef_type="c+cl", add_base_loss=True),
    "full_only_c": dict(loss=ALL_LOSS, ef_type="only_c"),
    "stages": dict(loss=ALL_LOSS),
})
STAGED = ("stages",)
# file -> the configs it stores: every term alone where the file stays under the cap
FILES = {
    "b1_l1_8x8": tuple(CONFIGS),
    "b2_l3_9x10": ("default", "full_c_cl_base1"),
    "at_threshold": ("compensation", "default", "full_c_cl_base1", "full_only_c"),
    "zero_gt": ("match", "ef", "default", "full_c_cl_base1", "full_only_c"),
    "zero_pred": ("norml1", "norml2", "ef", "match", "default", "full_c_cl_base1"),
}


def cases():
    """name -> (pred, gt, second stage or None): inputs from sparse(...), so they hold exact zeros; magnitudes far below
    a spread of 80 along l (match_low == 0)."""
    from make_voxlosses_goldens import sparse
    rng = np.random.default_rng(977)
    out = {}
    s = (1, 1, 20, 8, 8)                  # D = 10 = 1 mod 3: the padded last 3-window; one 8-window and two tail planes
    out["b1_l1_8x8"] = (sparse(rng, s, 0.5, 0.5), sparse(rng, s, 0.5, 0.5), sparse(rng, s, 0.3, 0.5))
    s = (2, 3, 20, 9, 10)                 # D = 30 = 0 mod 3: the last plane in no 3-window; ragged H, W; batch-total counts
    out["b2_l3_9x10"] = (sparse(rng, s, 2.0, 0.5), sparse(rng, s, 2.0, 0.5), None)
    s = (1, 2, 20, 9, 12)
    p, g = sparse(rng, s, 0.02, 0.5), sparse(rng, s, 0.02, 0.5)
    thr = np.float32(0.01)
    above = np.nextafter(thr, np.float32(1))
    p.reshape(-1)[::7] = thr
    p.reshape(-1)[3::11] = above
    g.reshape(-1)[::5] = thr
    g.reshape(-1)[2::13] = above
    out["at_threshold"] = (p, g, None)
    s = (1, 3, 20, 8, 10)
    out["zero_gt"] = (sparse(rng, s, 0.2, 0.6), np.zeros(s, np.float32), None)
    s = (1, 2, 20, 8, 8)                  # the norml2 zero rule and sign(0)
    out["zero_pred"] = (np.zeros(s, np.float32), sparse(rng, s, 0.4, 0.5), None)
    return out


def reference_grads(M, calc, preds, gt, double, loss, ef_type="c+cl", add_base_loss=False):
    """The reference's autograd gradient of its total with respect to every stage, as numpy arrays."""
    hp = SimpleNamespace(loss=list(loss), ef_type=ef_type, add_base_loss=add_base_loss, alpha_pyramid=1000, alpha_ef=0.5,
                         alpha_efc=5, alpha_match=0.5, alpha_compensation=1, alpha_pt=1, alpha_norm=1e-5)
    stub = SimpleNamespace(hparams=hp, ef_loss=torch.nn.MSELoss(),
                           loss_function={"pyramid": M.Pyramid3dLoss(add_base_loss=add_base_loss),
                                          "pt": M.PyramidTemporalLoss(), "match": M.MatchLoss(),
                                          "compensation": M.CompensationLoss()})
    cast = (lambda a: torch.from_numpy(a).double()) if double else (lambda a: torch.from_numpy(a).clone())
    stages = [cast(p).requires_grad_() for p in preds]
    # (a copy of the list: calculate_loss replaces the entries of the one it is given)
    total, _ = calc(stub, {"voxels": cast(gt)}, {"voxels": list(stages) if len(stages) > 1 else stages[0]})
    total.backward()
    return [s.grad.numpy() for s in stages]


def main(out_dir):
    from make_voxlosses_goldens import reference_calculate_loss, reference_losses
    os.makedirs(out_dir, exist_ok=True)
    M, calc = reference_losses(), reference_calculate_loss()
    all_cases = cases()
    assert set(all_cases) == set(FILES)
    for name, (p, g, p2) in all_cases.items():
        assert all(s["match_low"] == 0 for s in R.batch_stats(p, g)), name
        arrays = {"pred": p, "gt": g}
        for cfg in FILES[name]:
            preds = [p]
            if cfg in STAGED:
                assert p2 is not None and all(s["match_low"] == 0 for s in R.batch_stats(p2, g)), name
                arrays["pred2"] = p2
                preds.append(p2)
            g64 = reference_grads(M, calc, preds, g, True, **CONFIGS[cfg])
            g32 = reference_grads(M, calc, preds, g, False, **CONFIGS[cfg])
            for i, (a, b) in enumerate(zip(g64, g32)):
                key = cfg if i == 0 else f"{cfg}_p2"
                assert a.dtype == np.float64 and b.dtype == np.float32
                arrays[f"ref64_grad_{key}"] = a
                arrays[f"ref32_dev_{key}"] = np.abs(b.astype(np.float64) - a).max()
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(path, size)
        assert size <= SIZE_CAP, (path, size)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".voxlossgrads"))
