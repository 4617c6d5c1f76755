"""CPU side of the trainable last decoder convolution (include/v2ce_hip_convgrad.h, last_conv.py): the numpy restatement
(tests/last_conv_ref.py) against the reference block's own forward and autograd (tests/golden/.lastconv/), the export
tuple against its header, and what the C ABI and the Python layer refuse without a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import last_conv_ref as R
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY, MARGIN, SIZE_CAP
from v2ce_toolbox_amd import finetune, hip, last_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".lastconv")
LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
BAD_ARG, WORKSPACE = -1, -4


load = R.load_case


def test_goldens_are_the_recipes_files_and_small():
    want = [f"{n}{s}.npz" for n in CASES for s in (("", ".truth") if n in KERNEL_ONLY else ("", ".plain", ".layer"))]
    files = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
    assert sorted(os.path.basename(p) for p in files) == sorted(want)
    for p in files:
        assert os.path.getsize(p) <= SIZE_CAP, p
    for name, (B, L, H, W) in CASES.items():
        z = load(name)
        for k in ("t", "y", "upstream"):
            assert z[k].shape == (B, 32, L, H, W) and z[k].dtype == np.float32, (name, k)
        assert z["ref64_dM"].shape == (32, 32, 3, 3, 3) and z["ref64_d_shift"].shape == (32,)
        assert all(z[k].dtype == np.float64 for k in z if k.startswith(("ref64", "abs_terms", "ref32_dev"))), name
        if name not in KERNEL_ONLY:
            assert z["weight_bar"].shape == (32, 32, 3, 3, 3) and z["u"].shape == (32,) and z["v"].shape == (864,)
            assert z["ref64_d_weight_bar"].shape == (32, 32, 3, 3, 3) and z["ref64_dM_plain"].shape == (32, 32, 3, 3, 3)
    B, L, H, W = CASES[KERNEL_ONLY[0]]
    assert B * L * H * W > hip.WGRAD_CHAIN


def test_chain_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", "v2ce_hip_convgrad.h")).read()
    m = re.search(r"#define\s+V2CE_WGRAD_CHAIN\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.WGRAD_CHAIN and hip.WGRAD_CHAIN <= 4096


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_weight_gradient_matches_torch_f64(name):
    z = load(name)
    g = R.wgrad(z["t"], z["y"], z["upstream"])
    for got, key in ((g["d_weight"], "ref64_dM"), (g["d_shift"], "ref64_d_shift"), (g["abs_weight"], "abs_terms_dM"),
                     (g["abs_shift"], "abs_terms_d_shift")):
        assert np.abs(got - z[key]).max() <= 1e-12 * max(np.abs(z[key]).max(), 1e-300), key
    if name not in KERNEL_ONLY:
        p = R.wgrad(z["t"], None, z["upstream"])
        assert np.abs(p["d_weight"] - z["ref64_dM_plain"]).max() <= 1e-12 * np.abs(z["ref64_dM_plain"]).max()
        assert np.abs(p["d_shift"] - z["ref64_d_shift_plain"]).max() <= 1e-12 * np.abs(z["ref64_d_shift_plain"]).max()
        assert np.allclose(p["abs_weight"], z["abs_terms_dM_plain"], rtol=1e-12, atol=0)
    if name == "inactive":
        assert not z["ref64_dM"].any() and not z["ref64_d_shift"].any() and not z["y"].any()
    if name == "b1_l1_1x1":                          # only the centre tap sees the single position
        nz = z["ref64_dM_plain"].reshape(32, 32, 27).any(axis=(0, 1))
        assert nz.tolist() == [k == 13 for k in range(27)]


@pytest.mark.parametrize("name", LAYER_CASES)
def test_restated_layer_matches_the_reference_block(name):
    z = load(name)
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    assert np.abs(u1 - z["ref64_u_after"]).max() <= 1e-14 and np.abs(v1 - z["ref64_v_after"]).max() <= 1e-14
    u32, v32 = R.power_iteration(z["weight_bar"], z["u"], z["v"], np.float32)
    assert np.abs(u32 - z["ref32_u_after"]).max() <= 1e-6 and np.abs(v32 - z["ref32_v_after"]).max() <= 1e-6
    W, sigma, scale, shift = R.effective(z["weight_bar"], u1, v1, z["bn_weight"], z["bn_bias"], z["running_mean"],
                                         z["running_var"], z["eps"])
    feat, pre = R.forward(z["t"], z["res"], W, scale, shift)
    assert np.abs(feat - z["ref64_feat"]).max() <= 1e-12 * max(1.0, np.abs(z["ref64_feat"]).max())
    nz = pre[pre != 0]
    assert np.abs(nz).min() >= MARGIN                               # the mask is unambiguous
    assert np.array_equal(z["y"] > 0, pre > 0) and np.array_equal(z["y"], z["ref64_feat"].astype(np.float32))
    g = R.param_grads(z["ref64_dM"], z["ref64_d_shift"], z["weight_bar"], u1, v1, sigma, scale, z["running_mean"],
                      z["running_var"], z["eps"])
    for k in ("d_weight_bar", "d_bn_weight", "d_bn_bias"):
        want = z[f"ref64_{k}"]
        err = np.abs(g[k] - want).max()
        assert err <= 1e-11 * max(np.abs(want).max(), 1e-300), (k, err)
        # two-sided: rounded to f32 it is no farther from the f64 run than the reference's own f32 run, plus one rounding
        err32 = np.abs(g[k].astype(np.float32).astype(np.float64) - want).max()
        assert err32 <= float(z[f"ref32_dev_{k}"]) + 2.0 ** -23 * np.abs(want).max(), (k, err32)
    if name != "inactive":
        assert np.abs(z["ref64_d_weight_bar"]).max() > 0 and (z["y"] == 0).mean() > 0.1


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "v2ce_hip_convgrad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_convgrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVGRAD_EXPORTS) and len(set(hip.CONVGRAD_EXPORTS)) == len(hip.CONVGRAD_EXPORTS)
    for other in (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS):
        assert not set(hip.CONVGRAD_EXPORTS) & set(other)
    for other in ("v2ce_hip.h", "v2ce_hip_grad.h", "v2ce_hip_train.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(s in text for s in syms), other


def test_size_queries_and_refusals_without_gpu():
    L = hip.lib()
    q, f = L.v2ce_conv32_wgrad_workspace_bytes, L.v2ce_conv32_wgrad
    per_wg = (27 * 32 * 32 + 32) * 8
    assert q(1, 1, 1, 1, 1, 0) == (per_wg + 255) // 256 * 256
    assert q(2, 3, 5, 7, 7, 0) >= 2 * 3 * 3 * per_wg               # one workgroup per tile of 2 x 64 positions
    assert q(1, 3, 20, 70, 96, 1) == q(1, 1, 1, 1, 1, 0) and q(1, 3, 20, 70, 96, 7) >= 7 * per_wg > q(1, 3, 20, 70, 96, 6)
    assert q(1, 3, 20, 70, 96, 1000) == q(1, 3, 20, 70, 96, 0)     # a cap above the kernel's choice changes nothing
    assert q(4, 16, 260, 346, 352, 0) == q(1, 16, 260, 346, 352, 0) == (256 * per_wg + 255) // 256 * 256
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
    for bad in ((a + 4, a, a), (a, a + 8, a), (a, a, a + 4)):
        assert f(*bad, *d, a, a, a, 1 << 30, 0, None) == BAD_ARG
        assert b"16-byte" in L.v2ce_last_error()
    assert f(a, a, a, *d, a, a, a + 4, 1 << 30, 0, None) == BAD_ARG
    assert b"8-byte" in L.v2ce_last_error()
    assert f(a, a, a, *d, a, a, a, q(*d, 0) - 4, 0, None) == WORKSPACE
    assert f(a, None, a, *d, a, None, a, q(*d, 3) - 4, 3, None) == WORKSPACE
    assert f(a, a, a, *d, a, a, a, q(*d, 3), 0, None) == WORKSPACE  # sized for a capped grid, called without the cap


def c16(B=1, L=2, H=4, W=5):
    t = torch.zeros(B, L, 2, H, W, 16)
    t.lw = W
    return t


def test_python_refusals_without_gpu():
    x = c16()
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_conv.conv32_wgrad(x, x, x)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_conv.conv32_wgrad(x, None, x)
    with pytest.raises(ValueError, match="want"):
        last_conv.conv32_wgrad(x, x, x, want=())
    with pytest.raises(ValueError, match="want"):
        last_conv.conv32_wgrad(x, x, x, want=("weight", "bias"))
    with pytest.raises(ValueError, match="max_workgroups"):
        last_conv.conv32_wgrad(x, x, x, max_workgroups=-1)
    with pytest.raises(ValueError, match="from_model"):
        last_conv.LastConv()(x, x)
    layer = last_conv.LastConv()
    assert [n for n, _ in layer.named_parameters()] == ["weight_bar", "bn_weight", "bn_bias"]
    assert all(p.requires_grad for p in layer.parameters())
    assert layer.weight_bar.shape == (32, 32, 3, 3, 3) and layer.weight_u.shape == (32,) and layer.weight_v.shape == (864,)
    with pytest.raises(ValueError, match="train"):
        finetune.fit_tail(None, None, None, train=("pred", "conv1"), steps=1, lr=1e-3)
    with pytest.raises(ValueError, match="train"):
        finetune.fit_tail(None, None, None, train=(), steps=1, lr=1e-3)
    assert finetune.build_parser().parse_args(["--gt_events", "e.npz"]).train == "head"
    assert finetune.build_parser().parse_args(["--gt_events", "e.npz", "--train", "tail"]).train == "tail"


def test_effective_weights_follow_the_reference_iteration():
    z = load("b2_l3_5x7")
    layer = last_conv.LastConv()
    with torch.no_grad():
        for name, key in (("weight_bar", "weight_bar"), ("weight_u", "u"), ("weight_v", "v"), ("bn_weight", "bn_weight"),
                          ("bn_bias", "bn_bias"), ("running_mean", "running_mean"), ("running_var", "running_var")):
            getattr(layer, name).copy_(torch.from_numpy(z[key]))
        layer.eps.fill_(float(z["eps"]))
    W, scale, shift = layer.effective()
    assert W.requires_grad and scale.requires_grad and shift.requires_grad
    assert np.abs(layer.weight_u.numpy() - z["ref32_u_after"]).max() <= 1e-6
    assert np.abs(layer.weight_v.numpy() - z["ref32_v_after"]).max() <= 1e-6
    u1, v1 = R.power_iteration(z["weight_bar"], z["u"], z["v"])
    W64, sigma, scale64, shift64 = R.effective(z["weight_bar"], u1, v1, z["bn_weight"], z["bn_bias"], z["running_mean"],
                                               z["running_var"], z["eps"])
    assert np.abs(W.detach().numpy() - W64).max() <= 1e-6 * np.abs(W64).max()
    assert np.abs(scale.detach().numpy() - scale64).max() <= 1e-6 and np.abs(shift.detach().numpy() - shift64).max() <= 1e-6
    # torch's autograd through sigma, rsqrt and the affine forms gives the closed forms of the restatement
    dM, dsh = torch.from_numpy(z["ref64_dM"]).float(), torch.from_numpy(z["ref64_d_shift"]).float()
    dW = scale.detach().view(32, 1, 1, 1, 1) * dM
    d_scale = (W.detach() * dM).sum(dim=(1, 2, 3, 4))
    torch.autograd.backward([W, scale, shift], [dW, d_scale, dsh])
    for got, k in ((layer.weight_bar.grad, "d_weight_bar"), (layer.bn_weight.grad, "d_bn_weight"), (layer.bn_bias.grad, "d_bn_bias")):
        want = z[f"ref64_{k}"]
        assert np.abs(got.numpy() - want).max() <= 2e-5 * np.abs(want).max(), k


def test_from_model_and_write_back_touch_the_layer_only():
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    layer = last_conv.LastConv.from_model(m)
    inner, bn = m.UNet.decoders[-1].conv2.module, m.UNet.decoders[-1].bn2
    assert torch.equal(layer.weight_bar.detach(), inner.weight_bar) and torch.equal(layer.weight_u, inner.weight_u)
    assert torch.equal(layer.bn_weight.detach(), bn.weight) and torch.equal(layer.running_var, bn.running_var)
    with torch.no_grad():
        layer.weight_bar.add_(1.0)
        layer.bn_bias.sub_(2.0)
        layer.weight_u.mul_(0.5)
    m._prep = {"stale": True}
    layer.write_back(m)
    assert m._prep is None
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    pre = "UNet.decoders.3."
    assert changed == {pre + "conv2.module.weight_bar", pre + "conv2.module.weight_u", pre + "bn2.bias"}
    assert not inner.weight_bar.requires_grad
