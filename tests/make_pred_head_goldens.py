"""Recipe of tests/golden/.predhead/*.npz: inputs of the prediction head with the REFERENCE layer's own results.

The reference's ``ConvLayer3D(32, Cout, 1, activation='relu', norm=None)`` (train/scripts/model/submodules.py:79-118,
built at unet_2layer.py:364) is loaded by path, as tests/make_voxlossgrads_goldens.py loads the reference's losses; the
package around it is not executed (it imports pytorch_lightning).  Stored per file:
  feat [B, 32, L, H, W], weight [Cout, 32, 1, 1, 1], bias [Cout], upstream [B, Cout, L, H, W] as f32;
  ref64_y, ref64_d_weight, ref64_d_bias, ref64_d_feat: the layer's forward and autograd on ``.double()`` inputs;
  ref32_dev_<y, d_weight, d_bias, d_feat>: max |f32 run - f64 run| of the same layer, the reference's own rounding;
  abs_terms_d_weight [Cout, 32], abs_terms_d_bias [Cout]: the sum of |terms| of each element, f64.
The maker asserts that the f32 and f64 pre-activations agree in sign everywhere and that a non-zero pre-activation is at
least 1e-4 from 0, so the relu mask is unambiguous.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_pred_head_goldens.py [out_dir]   (default tests/golden/.predhead; V2CE_REFERENCE_ROOT names the tree)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
SIZE_CAP = 300_000
MARGIN = 1e-4
# name -> (B, L, H, W, Cout)
CASES = {
    "b1_l1_1x1": (1, 1, 1, 1, 20),
    "b2_l3_5x7": (2, 3, 5, 7, 20),
    "b1_l2_3x70": (1, 2, 3, 70, 20),          # the activation pitch pads 70 to 96
    "b1_l1_9x33": (1, 1, 9, 33, 20),
    "zero_preact": (1, 2, 5, 9, 20),          # positions with all-zero features and a zero bias: y == 0 exactly
    "cout_1": (1, 2, 5, 9, 1),
    "cout_32": (1, 2, 4, 9, 32),
    "negative_all": (1, 2, 5, 9, 20),         # no unit is active
}


def reference_layer_class():
    pkg = types.ModuleType("ref_model")
    pkg.__path__ = [os.path.join(REF, "train", "scripts", "model")]
    sys.modules["ref_model"] = pkg
    return importlib.import_module("ref_model.submodules").ConvLayer3D


def inputs(name):
    """Seeded f32 inputs of a case; values on a coarse grid away from a zero pre-activation (checked in main)."""
    B, L, H, W, cout = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 4242)
    feat = rng.standard_normal((B, 32, L, H, W)).astype(np.float32)
    feat[rng.random(feat.shape) < 0.2] = 0.0                    # relu outputs of the last block: exact zeros
    weight = (rng.standard_normal((cout, 32, 1, 1, 1)) * 0.2).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    upstream = rng.standard_normal((B, cout, L, H, W)).astype(np.float32)
    if name == "zero_preact":
        bias[::3] = 0.0
        feat[:, :, :, ::2, 1::3] = 0.0                          # whole positions without features
    if name == "negative_all":
        feat = np.abs(feat)
        weight = -np.abs(weight)
        bias = -np.abs(bias) - np.float32(0.01)
    return feat, weight, bias, upstream


def run(layer_cls, feat, weight, bias, upstream, double):
    cast = (lambda a: torch.from_numpy(a).double()) if double else (lambda a: torch.from_numpy(a).clone())
    layer = layer_cls(32, weight.shape[0], 1, activation="relu", norm=None)
    if double:
        layer = layer.double()
    with torch.no_grad():
        layer.conv3d.weight.copy_(cast(weight))
        layer.conv3d.bias.copy_(cast(bias))
    x = cast(feat).requires_grad_()
    pre = layer.conv3d(x)
    y = layer(x)
    y.backward(cast(upstream))
    return {"y": y.detach().numpy(), "d_weight": layer.conv3d.weight.grad.numpy().reshape(weight.shape[0], 32),
            "d_bias": layer.conv3d.bias.grad.numpy(), "d_feat": x.grad.numpy(), "pre": pre.detach().numpy()}


def main(out_dir):
    sys.path.insert(0, ROOT)
    from tests import pred_head_ref as R
    os.makedirs(out_dir, exist_ok=True)
    cls = reference_layer_class()
    for name in CASES:
        feat, weight, bias, upstream = inputs(name)
        r64, r32 = run(cls, feat, weight, bias, upstream, True), run(cls, feat, weight, bias, upstream, False)
        assert r64["y"].dtype == np.float64 and r32["y"].dtype == np.float32
        assert np.array_equal(np.sign(r64["pre"]), np.sign(r32["pre"])), name
        nz = r64["pre"][r64["pre"] != 0]
        assert nz.size == 0 or np.abs(nz).min() >= MARGIN, (name, np.abs(nz).min())
        own = R.grads(feat, r64["y"], upstream, weight)
        arrays = {"feat": feat, "weight": weight, "bias": bias, "upstream": upstream,
                  "abs_terms_d_weight": own["abs_weight"], "abs_terms_d_bias": own["abs_bias"]}
        for k in ("y", "d_weight", "d_bias", "d_feat"):
            arrays[f"ref64_{k}"] = r64[k]
            arrays[f"ref32_dev_{k}"] = np.abs(r32[k].astype(np.float64) - r64[k]).max()
        if name == "zero_preact":
            assert (r64["pre"] == 0).sum() > 10
        if name == "negative_all":
            assert not r64["y"].any() and not r64["d_weight"].any() and not r64["d_feat"].any()
        path = os.path.join(out_dir, f"{name}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(path, size)
        assert size <= SIZE_CAP, (path, size)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".predhead"))
