"""CPU side of the input gradient of the last decoder convolution and of the block's other two BatchNorms
(include/v2ce_hip_convdgrad.h, last_conv.py: conv32_dgrad, TailNorms; finetune.fit_tail_norms): the numpy restatement
(tests/last_conv_dgrad_ref.py) against torch's f64 conv3d input gradient and the reference block's own autograd
(tests/golden/.lastconv_dgrad/), the export tuple against its header, and what the C ABI and the Python layer refuse without
a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import last_conv_dgrad_ref as D
from tests import last_conv_ref as R
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY, MARGIN, SIZE_CAP
from v2ce_toolbox_amd import finetune, hip, last_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
BLOCK_GRADS = ("d_t", "d_res", "d_bn1_weight", "d_bn1_bias", "d_bnd_weight", "d_bnd_bias")
HEADERS = ("v2ce_hip.h", "v2ce_hip_grad.h", "v2ce_hip_train.h", "v2ce_hip_convgrad.h")
BAD_ARG, WORKSPACE = -1, -4


def test_goldens_are_the_recipes_files_and_small():
    files = sorted(glob.glob(os.path.join(D.GOLD, "*.npz")))
    stems = {re.sub(r"\.\d+\.npz$", "", os.path.basename(p)) for p in files}
    assert stems == {f"{n}.dx" for n in CASES} | {f"{n}.block" for n in LAYER_CASES}
    for p in files:
        assert re.search(r"\.(dx|block)\.\d+\.npz$", p) and os.path.getsize(p) <= SIZE_CAP, p
    for name, (B, L, H, W) in CASES.items():
        z = D.load_case(name)
        shape = (B, 32, L, H, W)
        assert z["weight"].shape == (32, 32, 3, 3, 3) and z["weight"].dtype == np.float32
        sfxs = ("",) if name in KERNEL_ONLY else ("", "_plain")
        for sfx in sfxs:
            assert z[f"ref64_dx{sfx}"].shape == shape and z[f"abs_terms_dx{sfx}"].shape == shape, name
            assert np.all(np.abs(z[f"ref64_dx{sfx}"]) <= z[f"abs_terms_dx{sfx}"] * (1 + 1e-12))
        assert all(z[k].dtype == np.float64 for k in z if k.startswith(("ref64", "abs_terms", "ref32_dev"))), name
        if name in KERNEL_ONLY:
            assert float(z["ref32_dev_dx"]) > 0 and "ref64_dx_plain" not in z and "c1" not in z
            continue
        for k in ("c1", "cd", "y_block"):
            assert z[k].shape == shape and z[k].dtype == np.float32, (name, k)
        assert z["ref64_d_t"].shape == shape and z["ref64_d_res"].shape == shape
        for bn in ("bn1", "bnd"):
            for q in ("weight", "bias", "mean", "var"):
                assert z[f"{bn}_{q}"].shape == (32,) and z[f"{bn}_{q}"].dtype == np.float32
            assert z[f"ref64_d_{bn}_weight"].shape == (32,) and z[f"ref64_d_{bn}_bias"].shape == (32,)
            assert np.abs(z[f"{bn}_weight"]).min() >= 0.5 and (z[f"{bn}_weight"] < 0).any()    # both signs, none near zero


def test_term_count_matches_the_header():
    text = open(os.path.join(ROOT, "include", "v2ce_hip_convdgrad.h")).read()
    m = re.search(r"#define\s+V2CE_DGRAD_TERMS\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.DGRAD_TERMS == 864 == 32 * 27


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_input_gradient_matches_torch_f64(name):
    z = D.load_case(name)
    g = D.dgrad(z["weight"], z["y"], z["upstream"])
    for got, key in ((g["d_x"], "ref64_dx"), (g["abs_x"], "abs_terms_dx")):
        assert np.abs(got - z[key]).max() <= 1e-12 * max(np.abs(z[key]).max(), 1e-300), key
    assert np.array_equal(g["d_res"], np.where(z["y"] > 0, z["upstream"], np.float32(0)).astype(np.float64))
    if name not in KERNEL_ONLY:
        p = D.dgrad(z["weight"], None, z["upstream"])
        assert np.abs(p["d_x"] - z["ref64_dx_plain"]).max() <= 1e-12 * np.abs(z["ref64_dx_plain"]).max()
        assert np.abs(p["abs_x"] - z["abs_terms_dx_plain"]).max() <= 1e-12 * np.abs(z["abs_terms_dx_plain"]).max()
        assert np.array_equal(p["d_res"], z["upstream"].astype(np.float64))
    if name == "inactive":
        assert not z["ref64_dx"].any() and not z["y"].any() and z["ref64_dx_plain"].any()
    if name == "b1_l1_1x1":                          # the single position sees the centre tap alone
        want = np.einsum("o,oc->c", z["upstream"].astype(np.float64).reshape(32), z["weight"].astype(np.float64)[:, :, 1, 1, 1])
        assert np.abs(z["ref64_dx_plain"].reshape(32) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", LAYER_CASES)
def test_restated_block_matches_the_reference_block(name):
    z = D.load_case(name)
    eps = float(z["eps"])
    z1, zd = D.normed(z["c1"], z["bn1_mean"], z["bn1_var"], eps), D.normed(z["cd"], z["bnd_mean"], z["bnd_var"], eps)
    t, res, pre1 = D.tail_forward(z1, zd, z["bn1_weight"], z["bn1_bias"], z["bnd_weight"], z["bnd_bias"])
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    W, sigma, scale, shift = R.effective(z["weight_bar"], u1, v1, z["bn_weight"], z["bn_bias"], z["running_mean"],
                                         z["running_var"], eps)
    feat, pre = R.forward(t, res, W, scale, shift)
    for q in (pre1, pre):
        assert np.abs(q[q != 0]).min() >= MARGIN                   # both masks are unambiguous
    assert np.array_equal(z["y_block"] > 0, pre > 0) and np.array_equal(z["y_block"], feat.astype(np.float32))
    g = D.dgrad(scale[:, None, None, None, None] * W, z["y_block"], z["upstream"])
    tg = D.tail_grads(z1, zd, z["bn1_weight"], z["bn1_bias"], g["d_x"], g["d_res"])
    got = {"d_t": g["d_x"], "d_res": g["d_res"], **{k: tg[k] for k in BLOCK_GRADS[2:]}}
    for k in BLOCK_GRADS:
        want = z[f"ref64_{k}"]
        err = np.abs(got[k] - want).max()
        assert err <= 1e-11 * max(np.abs(want).max(), 1e-300), (k, err)
        # two-sided: rounded to f32 it is no farther from the f64 run than the reference's own f32 run, plus one rounding
        err32 = np.abs(got[k].astype(np.float32).astype(np.float64) - want).max()
        assert err32 <= float(z[f"ref32_dev_{k}"]) + 2.0 ** -23 * np.abs(want).max(), (k, err32)
    if name == "inactive":
        assert not any(z[f"ref64_{k}"].any() for k in BLOCK_GRADS) and not z["y_block"].any()
    else:
        assert all(np.abs(z[f"ref64_{k}"]).max() > 0 for k in BLOCK_GRADS) and 0.2 < (pre1 > 0).mean() < 0.8


def declared_symbols(header="v2ce_hip_convdgrad.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_convdgrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVDGRAD_EXPORTS) and len(set(hip.CONVDGRAD_EXPORTS)) == len(hip.CONVDGRAD_EXPORTS)
    for other in (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS):
        assert not set(hip.CONVDGRAD_EXPORTS) & set(other)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "v2ce_hip_convdgrad.h"]
    assert set(HEADERS) <= {os.path.basename(p) for p in others}
    for other in others:
        assert not any(s in open(other).read() for s in syms), other


def test_size_queries_and_refusals_without_gpu():
    L = hip.lib()
    q, f = L.v2ce_conv32_dgrad_workspace_bytes, L.v2ce_conv32_dgrad
    packed = 27 * 32 * 32 * 4                                       # the repacked weight: the grid needs nothing
    assert q(1, 1, 1, 1, 1, 0) == packed and packed % 256 == 0
    assert q(2, 3, 5, 7, 7, 0) == q(1, 3, 20, 70, 96, 1) == q(1, 3, 20, 70, 96, 7) == q(4, 16, 260, 346, 352, 0) == packed
    assert q(0, 3, 5, 7, 7, 0) == 0 and q(2, 0, 5, 7, 7, 0) == 0 and q(2, 3, 0, 7, 7, 0) == 0 and q(2, 3, 5, 0, 7, 0) == 0
    assert q(2, 3, 5, 7, 6, 0) == 0                                 # pitch < W
    assert q(2, 3, 5, 7, 7, -1) == 0
    assert q(4096, 4096, 16, 16, 16, 0) == 0                        # 2^32 positions
    d = (2, 3, 5, 7, 7)
    # refused before anything is launched (the addresses below are never dereferenced)
    assert f(None, None, None, *d, None, None, None, 0, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    assert f(None, None, None, 2, 3, 5, 7, 6, None, None, None, 0, 0, None) == BAD_ARG
    assert b"pitch" in L.v2ce_last_error()
    a = 4096                                                        # aligned stand-ins for device addresses
    assert f(a, a, a, *d, None, None, a, 1 << 30, 0, None) == BAD_ARG
    assert b"no output" in L.v2ce_last_error()
    assert f(a, a, a, *d, a, a, a, 1 << 30, -1, None) == BAD_ARG
    assert b"max_workgroups" in L.v2ce_last_error()
    assert f(a, a, None, *d, a, a, a, 1 << 30, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
    assert f(None, a, a, *d, a, a, a, 1 << 30, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
    for bad in ((a + 8, a, a, a), (a, a + 4, a, a), (a, a, a + 4, a), (a, a, a, a + 8)):     # y, upstream, d_x, d_res
        assert f(a, bad[0], bad[1], *d, bad[2], bad[3], a, 1 << 30, 0, None) == BAD_ARG
        assert b"16-byte" in L.v2ce_last_error()
    assert f(a + 2, a, a, *d, a, a, a, 1 << 30, 0, None) == BAD_ARG
    assert b"4-byte" in L.v2ce_last_error()
    assert f(a, a, a, *d, a, a, a + 4, 1 << 30, 0, None) == BAD_ARG
    assert b"8-byte" in L.v2ce_last_error()
    assert f(a, a, a, *d, a, a, a, q(*d, 0) - 4, 0, None) == WORKSPACE
    assert f(a, None, a, *d, a, None, a, q(*d, 3) - 4, 3, None) == WORKSPACE
    assert f(a, None, a, *d, None, a, a, 0, 0, None) == WORKSPACE
    assert b"too small" in L.v2ce_last_error()


def c16(B=1, L=2, H=4, W=5):
    t = torch.zeros(B, L, 2, H, W, 16)
    t.lw = W
    return t


def test_python_refusals_without_gpu():
    x, w = c16(), torch.zeros(32, 32, 3, 3, 3)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_conv.conv32_dgrad(w, x, x)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_conv.conv32_dgrad(w, None, x)
    with pytest.raises(ValueError, match="want"):
        last_conv.conv32_dgrad(w, x, x, want=())
    with pytest.raises(ValueError, match="want"):
        last_conv.conv32_dgrad(w, x, x, want=("x", "weight"))
    with pytest.raises(ValueError, match="want"):
        last_conv.conv32_dgrad(w, x, x, want=("x", "x"))
    with pytest.raises(ValueError, match="max_workgroups"):
        last_conv.conv32_dgrad(w, x, x, max_workgroups=-1)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_conv.TailNorms()(x, x)
    assert last_conv.DGRAD_WANT == ("x", "res")


def test_tail_norms_parameters_and_model_round_trip():
    layer = last_conv.TailNorms()
    assert [n for n, _ in layer.named_parameters()] == ["bn1_weight", "bn1_bias", "bnd_weight", "bnd_bias"]
    assert all(p.requires_grad and p.shape == (32,) for p in layer.parameters()) and not list(layer.buffers())
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    layer = last_conv.TailNorms.from_model(m)
    blk = m.UNet.decoders[-1]
    assert torch.equal(layer.bn1_weight.detach(), blk.bn1.weight) and torch.equal(layer.bnd_bias.detach(), blk.downsample[1].bias)
    with torch.no_grad():
        layer.bn1_bias.add_(1.0)
        layer.bnd_weight.mul_(0.0)                                  # a zero weight is a legal value
    m._prep = {"stale": True}
    layer.write_back(m)
    assert m._prep is None
    changed = {k for k, v in m.state_dict().items() if not torch.equal(before[k], v)}
    assert changed == {"UNet.decoders.3.bn1.bias", "UNet.decoders.3.downsample.1.weight"}


def test_fit_tail_norms_train_validation_and_the_parser():
    assert finetune.TAIL_NORM_GROUPS == ("pred", "conv2", "bn2", "bn1", "bnd") and finetune.TAIL_GROUPS == ("pred", "conv2", "bn2")
    for bad in (("pred", "conv1"), (), ("bn1", "bn1"), ("bn1", "bn3")):
        with pytest.raises(ValueError, match="train"):
            finetune.fit_tail_norms(None, None, None, train=bad, steps=1, lr=1e-3)
    with pytest.raises(ValueError, match="train"):                  # fit_tail's own refusal is untouched
        finetune.fit_tail(None, None, None, train=("pred", "bn1"), steps=1, lr=1e-3)
    with pytest.raises(ValueError, match="optimizer"):
        finetune.fit_tail_norms(None, None, None, train=("bn1",), steps=1, lr=1e-3, optimizer="lbfgs")
    parse = finetune.build_parser().parse_args
    assert parse(["--gt_events", "e.npz"]).train == "head"
    assert parse(["--gt_events", "e.npz", "--train", "tail"]).train == "tail"
    assert parse(["--gt_events", "e.npz", "--train", "tail_norms"]).train == "tail_norms"
    with pytest.raises(SystemExit):
        parse(["--gt_events", "e.npz", "--train", "norms"])
