"""CPU side of the trainable prediction head (include/v2ce_hip_train.h, pred_head.py): the numpy restatement
(tests/pred_head_ref.py) against the reference layer's own forward and autograd (tests/golden/.predhead/), the export
tuple against its header, and what the C ABI and the Python layer refuse without a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import pred_head_ref as R
from tests.make_pred_head_goldens import CASES, MARGIN, SIZE_CAP
from v2ce_toolbox_amd import hip, pred_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".predhead")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
name_of = lambda p: os.path.basename(p)[:-4]
BAD_ARG, WORKSPACE = -1, -4
OUTPUTS = ("y", "d_weight", "d_bias", "d_feat")


def test_goldens_are_the_recipes_files_and_small():
    assert [name_of(p) for p in GOLDENS] == sorted(CASES)
    keys = {"feat", "weight", "bias", "upstream", "abs_terms_d_weight", "abs_terms_d_bias"}
    keys |= {f"ref64_{k}" for k in OUTPUTS} | {f"ref32_dev_{k}" for k in OUTPUTS}
    for p in GOLDENS:
        assert os.path.getsize(p) <= SIZE_CAP, p
        z = np.load(p)
        assert set(z.files) == keys, p
        B, L, H, W, cout = CASES[name_of(p)]
        assert z["feat"].shape == (B, 32, L, H, W) and z["upstream"].shape == (B, cout, L, H, W)
        assert z["weight"].shape == (cout, 32, 1, 1, 1) and z["bias"].shape == (cout,)
        assert all(z[k].dtype == np.float32 for k in ("feat", "weight", "bias", "upstream"))
        assert all(z[k].dtype == np.float64 for k in z.files if k.startswith(("ref", "abs")))


def test_fixtures_exercise_what_they_are_for():
    z = {name_of(p): np.load(p) for p in GOLDENS}
    assert R.pitch_of(70) == 96 and R.pitch_of(33) == 33
    for name, f in z.items():                                      # the mask is unambiguous
        pre = np.einsum("bclhw,oc->bolhw", f["feat"].astype(np.float64), f["weight"].astype(np.float64).reshape(-1, 32))
        pre += f["bias"].astype(np.float64)[None, :, None, None, None]
        assert np.abs(pre[pre != 0]).min() >= MARGIN, name
        assert (f["feat"] == 0).mean() > 0.1, name
    zp = z["zero_preact"]
    assert (zp["ref64_y"] == 0).any() and not zp["feat"][:, :, :, ::2, 1::3].any() and (zp["bias"] == 0).any()
    # units with an exactly zero pre-activation (no features, zero bias): nothing flows through them, so the gradient of
    # such a position is that of its other units alone
    pre = np.einsum("bclhw,oc->bolhw", zp["feat"].astype(np.float64), zp["weight"].astype(np.float64).reshape(-1, 32))
    pre += zp["bias"].astype(np.float64)[None, :, None, None, None]
    at_zero = pre == 0
    assert at_zero.sum() > 10 and zp["upstream"][at_zero].all()
    m = np.where(pre > 0, zp["upstream"].astype(np.float64), 0.0)
    want = np.einsum("bolhw,oc->bclhw", m, zp["weight"].astype(np.float64).reshape(-1, 32))
    assert np.abs(want - zp["ref64_d_feat"]).max() <= 1e-12
    na = z["negative_all"]
    assert not na["ref64_y"].any() and not na["ref64_d_weight"].any() and not na["ref64_d_bias"].any()
    assert z["cout_1"]["weight"].shape[0] == 1 and z["cout_32"]["weight"].shape[0] == 32


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_restatement_matches_the_reference_layer(path):
    z = np.load(path)
    y = R.forward(z["feat"], z["weight"], z["bias"])
    g = R.grads(z["feat"], y, z["upstream"], z["weight"])
    got = {"y": y, "d_weight": g["d_weight"], "d_bias": g["d_bias"], "d_feat": g["d_feat"]}
    for k in OUTPUTS:
        want = z[f"ref64_{k}"]
        assert got[k].shape == want.shape, k
        err = np.abs(got[k] - want)
        scale = np.abs(want).max()
        assert err.max() <= 1e-12 * max(scale, 1e-300), (k, err.max(), scale)
        # two-sided: rounded to f32 it is no farther from the f64 run than the reference's own f32 run, plus one rounding
        err32 = np.abs(got[k].astype(np.float32).astype(np.float64) - want).max()
        assert err32 <= float(z[f"ref32_dev_{k}"]) + 2.0 ** -23 * scale, (k, err32)
    # the mask from the f32-rounded output is the mask of the f64 output
    assert np.array_equal(R.masked(y.astype(np.float32), z["upstream"]), R.masked(y, z["upstream"]))
    assert np.allclose(g["abs_weight"], z["abs_terms_d_weight"], rtol=1e-12, atol=0)
    assert np.allclose(g["abs_bias"], z["abs_terms_d_bias"], rtol=1e-12, atol=0)


def test_layout_helpers_round_trip():
    rng = np.random.default_rng(3)
    f = rng.standard_normal((2, 32, 3, 4, 70)).astype(np.float32)
    c = R.to_c16(f, 96)
    assert c.shape == (2, 3, 2, 4, 96, 16) and np.isnan(c[..., 70:, :]).all() and not np.isnan(c[..., :70, :]).any()
    assert c[1, 2, 1, 3, 5, 7] == f[1, 16 + 7, 2, 3, 5]
    assert np.array_equal(R.from_c16(c, 70), f)
    y = rng.standard_normal((2, 20, 3, 4, 7))
    assert np.array_equal(R.from_dense(R.to_dense(y)), y) and R.to_dense(y).shape == (2, 3, 20, 4, 7)


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "v2ce_hip_train.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_train_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.TRAIN_EXPORTS) and len(set(hip.TRAIN_EXPORTS)) == len(hip.TRAIN_EXPORTS)
    assert not set(hip.TRAIN_EXPORTS) & set(hip.EXPORTS) and not set(hip.TRAIN_EXPORTS) & set(hip.GRAD_EXPORTS)
    for other in ("v2ce_hip.h", "v2ce_hip_grad.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(s in text for s in syms), other


def test_size_queries_and_refusals_without_gpu():
    L = hip.lib()
    fq, gq = L.v2ce_pred_head_fwd_workspace_bytes, L.v2ce_pred_head_grads_workspace_bytes
    for q in (fq, gq):
        assert q(2, 3, 20, 5, 7, 7) > 0 and q(1, 1, 1, 1, 1, 1) > 0 and q(1, 2, 32, 3, 70, 96) > 0
        assert q(2, 3, 0, 5, 7, 7) == 0 and q(2, 3, 33, 5, 7, 7) == 0          # Cout 0 or 33
        assert q(0, 3, 20, 5, 7, 7) == 0 and q(2, 0, 20, 5, 7, 7) == 0 and q(2, 3, 20, 0, 7, 7) == 0
        assert q(2, 3, 20, 5, 0, 7) == 0
        assert q(2, 3, 20, 5, 7, 6) == 0                                      # pitch < W
        assert q(4096, 4096, 20, 16, 16, 16) == 0                             # 2^32 positions
    assert gq(2, 3, 20, 5, 7, 7) > fq(2, 3, 20, 5, 7, 7)                       # the partial sums
    # one workgroup per 128-position tile up to 512 workgroups: the workspace stops growing there
    assert gq(1, 1, 20, 1, 128 * 512, 128 * 512) == gq(1, 1, 20, 1, 128 * 4000, 128 * 4000) > gq(1, 1, 20, 1, 128 * 511, 128 * 511)
    d = (2, 3, 20, 5, 7, 7)
    # null pointers: refused before anything is launched (the addresses below are never dereferenced)
    assert L.v2ce_pred_head_fwd(None, None, None, *d, None, None, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    assert L.v2ce_pred_head_grads(None, None, None, None, *d, None, None, None, None, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    for cout in (0, 33):
        assert L.v2ce_pred_head_fwd(None, None, None, 2, 3, cout, 5, 7, 7, None, None, 0, None) == BAD_ARG
        assert b"Cout" in L.v2ce_last_error()
        assert L.v2ce_pred_head_grads(None, None, None, None, 2, 3, cout, 5, 7, 7, None, None, None, None, 0, None) == BAD_ARG
        assert b"Cout" in L.v2ce_last_error()
    a = 4096                                                                   # aligned stand-ins for device addresses
    assert L.v2ce_pred_head_grads(a, a, a, a, *d, None, None, None, a, 1 << 30, None) == BAD_ARG
    assert b"no output" in L.v2ce_last_error()
    assert L.v2ce_pred_head_grads(a + 4, a, a, a, *d, a, None, None, a, 1 << 30, None) == BAD_ARG
    assert b"16-byte" in L.v2ce_last_error()
    assert L.v2ce_pred_head_grads(a, a, a, a, *d, a, None, a + 8, a, 1 << 30, None) == BAD_ARG
    assert L.v2ce_pred_head_grads(a, a, a, a, *d, a, None, None, a + 4, 1 << 30, None) == BAD_ARG
    assert b"8-byte" in L.v2ce_last_error()
    assert L.v2ce_pred_head_grads(a, a, a, a, *d, a, None, None, a, gq(*d) - 4, None) == WORKSPACE
    assert L.v2ce_pred_head_fwd(a, a, a, *d, a, a, fq(*d) - 4, None) == WORKSPACE
    assert L.v2ce_pred_head_fwd(a + 8, a, a, *d, a, a, fq(*d), None) == BAD_ARG


def test_python_refusals_without_gpu():
    feat = torch.zeros(1, 2, 2, 4, 5, 16)
    w, b = torch.zeros(20, 32, 1, 1, 1), torch.zeros(20)
    y = torch.zeros(1, 2, 20, 4, 5)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        pred_head.pred_head_forward(feat, w, b)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        pred_head.pred_head_grads(feat, y, y, w)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        pred_head.PredHead()(feat)
    with pytest.raises(ValueError, match="want"):
        pred_head.pred_head_grads(feat, y, y, w, want=())
    with pytest.raises(ValueError, match="want"):
        pred_head.pred_head_grads(feat, y, y, w, want=("weight", "gamma"))
    with pytest.raises(ValueError):
        pred_head.PredHead(33)
    head = pred_head.PredHead()
    assert head.weight.shape == (20, 32, 1, 1, 1) and head.bias.shape == (20,)
    assert head.weight.requires_grad and head.bias.requires_grad
    assert [n for n, _ in head.named_parameters()] == ["weight", "bias"]


def test_from_model_and_write_back_touch_the_head_only():
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    head = pred_head.PredHead.from_model(m)
    assert torch.equal(head.weight.detach(), m.UNet.pred.conv3d.weight) and torch.equal(head.bias.detach(), m.UNet.pred.conv3d.bias)
    with torch.no_grad():
        head.weight.add_(1.0)
        head.bias.sub_(2.0)
    m._prep = {"stale": True}
    head.write_back(m)
    assert m._prep is None
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == {"UNet.pred.conv3d.weight", "UNet.pred.conv3d.bias"}
    assert torch.equal(after["UNet.pred.conv3d.weight"], before["UNet.pred.conv3d.weight"] + 1.0)
    assert not m.UNet.pred.conv3d.weight.requires_grad
    with pytest.raises(NotImplementedError):
        m.train()
