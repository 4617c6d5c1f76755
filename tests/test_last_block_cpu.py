"""CPU side of the trainable first half of the last decoder block (include/v2ce_hip_convupgrad.h, last_block.py): the
goldens' files, the numpy restatement (tests/last_block_ref.py) against torch's f64 weight gradients on the materialised
upsample + concat (tests/golden/.lastblock/), the export tuple against its header, and what the C ABI and the Python layer
refuse without a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import last_block_ref as R
from tests.make_last_block_goldens import CASES, KERNEL_ONLY, MARGIN, SIZE_CAP
from v2ce_toolbox_amd import finetune, hip, last_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".lastblock")
LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
HEADER = "v2ce_hip_convupgrad.h"
BAD_ARG, WORKSPACE = -1, -4

load = R.load_case


def test_goldens_are_the_recipes_files_and_small():
    want = [f"{n}{s}.npz" for n in CASES for s in R.SUFFIXES + (() if n in KERNEL_ONLY else R.LAYER_SUFFIXES)]
    files = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
    assert sorted(os.path.basename(p) for p in files) == sorted(want)
    for p in files:
        assert os.path.getsize(p) <= SIZE_CAP, p
    for name, (B, L, H, W) in CASES.items():
        z = load(name)
        assert z["x0"].shape == (B, 64, L, (H + 1) // 2, (W + 1) // 2) and z["x0"].dtype == np.float32, name
        for k in ("x1", "g1", "gd"):
            assert z[k].shape == (B, 32, L, H, W) and z[k].dtype == np.float32, (name, k)
        assert z["ref64_dW"].shape == z["abs_terms_dW"].shape == (32, 96, 3, 3, 3)
        assert z["ref64_dMd"].shape == z["abs_terms_dMd"].shape == (32, 96) and z["ref64_d_sum"].shape == (32,)
        assert all(z[k].dtype == np.float64 for k in z if k.startswith(("ref64", "abs_terms", "ref32_dev"))), name
        if name not in KERNEL_ONLY:
            assert all(z[k].dtype == np.float32 for k in R.PARAMS) and z["upstream"].shape == (B, 32, L, H, W)
            assert z["weight_bar1"].shape == z["ref64_d_weight_bar1"].shape == (32, 96, 3, 3, 3) and z["v1"].shape == (2592,)
            assert z["short_weight"].shape == z["ref64_d_short_weight"].shape == (32, 96, 1, 1, 1)
            assert z["weight_bar2"].shape == z["ref64_d_weight_bar2"].shape == (32, 32, 3, 3, 3) and z["v2"].shape == (864,)
            assert z["mask_t"].dtype == z["mask_y"].dtype == np.bool_ and z["mask_t"].shape == z["mask_y"].shape == (B, 32, L, H, W)
            assert all(z[f"ref64_{k}"].dtype == np.float64 and f"ref32_dev_{k}" in z for k in R.BLOCK_GRADS), name
    B, L, H, W = CASES[KERNEL_ONLY[0]]
    assert B * L * H * W > hip.UPWGRAD_CHAIN
    z = load(KERNEL_ONLY[0])
    assert float(z["ref32_dev_dW"]) > 0 and float(z["ref32_dev_dMd"]) > 0      # f32 sums of its terms do round
    assert not load("zero")["g1"].any() and not load("zero")["gd"].any()


def test_chain_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    m = re.search(r"#define\s+V2CE_UPWGRAD_CHAIN\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.UPWGRAD_CHAIN and hip.UPWGRAD_CHAIN <= 4096


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_weight_gradients_match_torch_f64(name):
    z = load(name)
    g = R.wgrad(z["x0"], z["x1"], z["g1"], z["gd"])
    for got, key in ((g["d_weight"], "ref64_dW"), (g["d_short"], "ref64_dMd"), (g["d_short_bias"], "ref64_d_sum"),
                     (g["abs_weight"], "abs_terms_dW"), (g["abs_short"], "abs_terms_dMd"),
                     (g["abs_short_bias"], "abs_terms_d_sum")):
        assert got.shape == z[key].shape
        assert np.abs(got - z[key]).max() <= 1e-12 * max(np.abs(z[key]).max(), 1e-300), key
    if name == "zero":
        assert not z["ref64_dW"].any() and not z["ref64_dMd"].any() and not z["ref64_d_sum"].any()
    if name == "b1_l1_1x1":                          # only the centre tap sees the single position
        nz = z["ref64_dW"].reshape(32, 96, 27).any(axis=(0, 1))
        assert nz.tolist() == [k == 13 for k in range(27)]
    if name == "b2_l3_5x7":
        # the padding is the upsampled tensor's: the last source row (h0 = 2) is output row 4 alone, so the tap kh = 2 of the
        # last output row sees nothing, although the source row below the one of output row 3 exists
        X = R.virtual_input(z["x0"], z["x1"])
        assert np.array_equal(X[:, :64, :, 4], z["x0"][:, :, :, 2][..., np.arange(7) >> 1]) and X.shape[3] == 5
        assert np.array_equal(X[:, :64, :, 2], X[:, :64, :, 3]) and not np.array_equal(X[:, :64, :, 3], X[:, :64, :, 4])


def test_the_centre_tap_of_the_restatement_is_the_shortcut():
    z = load("b2_l3_5x7")
    g = R.wgrad(z["x0"], z["x1"], z["gd"], z["gd"])
    assert np.array_equal(g["d_weight"][:, :, 1, 1, 1], g["d_short"])


@pytest.mark.parametrize("name", LAYER_CASES)
def test_restated_block_matches_the_reference_block(name):
    z = load(name)
    p = {k: z[k] for k in R.PARAMS}
    f = R.block_forward(z["x0"], z["x1"], p)
    for mine, theirs in (("u1a", "u1_after"), ("v1a", "v1_after"), ("u2a", "u2_after"), ("v2a", "v2_after")):
        assert np.abs(f[mine] - z[f"ref64_{theirs}"]).max() <= 1e-14, theirs
    from tests import last_conv_ref as R2
    for wb, u, v, k in (("weight_bar1", "u1", "v1", "1"), ("weight_bar2", "u2", "v2", "2")):
        u32, v32 = R2.power_iteration(z[wb], z[u], z[v], np.float32)
        assert np.abs(u32 - z[f"ref32_u{k}_after"]).max() <= 1e-6 and np.abs(v32 - z[f"ref32_v{k}_after"]).max() <= 1e-6
    for q in (f["pre1"], f["pre"]):                                     # both masks are unambiguous
        assert np.abs(q[q != 0]).min() >= MARGIN
    assert np.array_equal(z["mask_t"], f["pre1"] > 0) and np.array_equal(z["mask_y"], f["pre"] > 0)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    for k in R.BLOCK_GRADS:
        want = z[f"ref64_{k}"]
        err = np.abs(g[k] - want).max()
        assert g[k].shape == want.shape and err <= 1e-11 * max(np.abs(want).max(), 1e-300), (k, err)
        # two-sided: rounded to f32 it is no farther from the f64 run than the reference's own f32 run, plus one rounding
        err32 = np.abs(g[k].astype(np.float32).astype(np.float64) - want).max()
        assert err32 <= float(z[f"ref32_dev_{k}"]) + 2.0 ** -23 * np.abs(want).max(), (k, err32)
    # the kernel's raw outputs for the block's own (g1, gd) are what the closed forms take
    k = R.wgrad(z["x0"], z["x1"], g["g1"], g["gd"])
    cg = R.conv_grads(k["d_weight"], k["d_short"], k["d_short_bias"], z["weight_bar1"], f["u1a"], f["v1a"], f["sigma1"], f["rs1"], f["rsd"])
    assert all(np.array_equal(cg[n], g[n]) for n in ("d_weight_bar1", "d_short_weight", "d_short_bias"))
    e = R.conv_bounds(np.abs(k["d_weight"]), np.abs(k["d_short"]), np.abs(k["d_short_bias"]), z["weight_bar1"], f["u1a"], f["v1a"],
                      f["sigma1"], f["rs1"], f["rsd"])
    assert all(np.all(np.abs(cg[n]) <= e[n] * (1 + 1e-12) + 1e-300) for n in e)      # the bound's form dominates the value's
    if name == "zero":
        assert not any(z[f"ref64_{k}"].any() for k in R.BLOCK_GRADS) and not z["upstream"].any()
    else:
        assert all(np.abs(z[f"ref64_{k}"]).max() > 0 for k in R.BLOCK_GRADS)
        assert 0.2 < z["mask_t"].mean() < 0.8 and 0.2 < z["mask_y"].mean() < 0.8


def declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_symbols_of_the_convupgrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVUPGRAD_EXPORTS) and len(set(hip.CONVUPGRAD_EXPORTS)) == len(hip.CONVUPGRAD_EXPORTS)
    for other in (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS):
        assert not set(hip.CONVUPGRAD_EXPORTS) & set(other)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != HEADER]
    assert len(others) >= 5
    for other in others:
        assert not any(s in open(other).read() for s in syms), other
    # the header names the older entries by file only (their own tests look for their symbols in every other header)
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    assert not any(s in own for s in hip.CONVGRAD_EXPORTS + hip.CONVDGRAD_EXPORTS)


def test_size_queries_and_refusals_without_gpu():
    L = hip.lib()
    q, f = L.v2ce_convup_wgrad_workspace_bytes, L.v2ce_convup_wgrad
    per_wg = (28 * 32 * 32 + 32) * 8
    up = lambda n: (n + 255) // 256 * 256
    assert q(1, 1, 1, 1, 1, 1, 0) == up(3 * per_wg)
    assert q(2, 3, 5, 7, 7, 4, 0) == up(2 * 3 * 3 * 3 * per_wg)        # three workgroups per tile of 2 x 64 positions
    big = (1, 3, 20, 70, 96, 35)
    assert q(*big, 1) == q(*big, 3) == q(*big, 5) == q(1, 1, 1, 1, 1, 1, 0)     # one share
    assert q(*big, 7) == q(*big, 6) == up(6 * per_wg)
    assert q(*big, 1000) == q(*big, 0) == up(60 * 3 * per_wg)          # a cap above the kernel's choice changes nothing
    assert q(4, 16, 260, 346, 352, 173, 0) == q(1, 16, 260, 346, 352, 192, 0) == up(85 * 3 * per_wg)
    assert q(0, 3, 5, 7, 7, 4, 0) == 0 and q(2, 0, 5, 7, 7, 4, 0) == 0 and q(2, 3, 0, 7, 7, 4, 0) == 0 and q(2, 3, 5, 0, 7, 4, 0) == 0
    assert q(2, 3, 5, 7, 6, 4, 0) == 0                                  # pitch < W
    assert q(2, 3, 5, 7, 7, 3, 0) == 0 and q(2, 3, 5, 8, 8, 4, 0) > 0   # pitch0 < W0 = (W + 1) / 2
    assert q(2, 3, 5, 7, 7, 4, -1) == 0
    assert q(4096, 4096, 16, 16, 16, 8, 0) == 0                         # 2^32 positions
    assert q(1, 1 << 20, 1, 1 << 10, 1 << 14, 1 << 9, 0) == 0 and q(1, 1 << 20, 1, 1 << 10, 1 << 10, 1 << 14, 0) == 0   # a pitch
    d = (2, 3, 5, 7, 7, 4)
    a = 4096                                                            # aligned stand-ins for device addresses
    # refused before anything is launched (the addresses below are never dereferenced)
    assert f(None, None, None, None, *d, a, a, a, a, 1 << 30, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    assert f(a, a, a, a, 2, 3, 5, 7, 6, 4, a, a, a, a, 1 << 30, 0, None) == BAD_ARG
    assert b"pitch" in L.v2ce_last_error()
    assert f(a, a, a, a, 2, 3, 5, 7, 7, 3, a, a, a, a, 1 << 30, 0, None) == BAD_ARG
    assert b"pitch0" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, None, None, None, a, 1 << 30, 0, None) == BAD_ARG
    assert b"no output" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a, a, 1 << 30, -1, None) == BAD_ARG
    assert f(a, a, a, a, *d, a, a, a, None, 1 << 30, 0, None) == BAD_ARG            # no workspace
    # an input is needed exactly by the outputs that read it
    assert f(a, a, None, a, *d, a, a, a, a, 1 << 30, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()     # d_weight needs g1
    assert f(a, a, a, None, *d, None, a, None, a, 1 << 30, 0, None) == BAD_ARG      # d_short needs gd
    assert f(a, a, a, None, *d, None, None, a, a, 1 << 30, 0, None) == BAD_ARG      # d_short_bias needs gd
    assert f(None, a, a, a, *d, None, a, None, a, 1 << 30, 0, None) == BAD_ARG      # d_short needs x0
    assert f(a, None, a, a, *d, a, None, None, a, 1 << 30, 0, None) == BAD_ARG      # d_weight needs x1
    for bad in ((a + 4, a, a, a), (a, a + 8, a, a), (a, a, a + 4, a), (a, a, a, a + 12)):
        assert f(*bad, *d, a, a, a, a, 1 << 30, 0, None) == BAD_ARG
        assert b"16-byte" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a, a + 4, 1 << 30, 0, None) == BAD_ARG
    assert b"8-byte" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a, a, q(*d, 0) - 4, 0, None) == WORKSPACE
    # an input nothing needs may be NULL: these get as far as the workspace check
    assert f(a, a, a, None, *d, a, None, None, a, q(*d, 3) - 4, 3, None) == WORKSPACE
    assert f(a, a, None, a, *d, None, a, a, a, q(*d, 3) - 4, 3, None) == WORKSPACE
    assert f(None, None, None, a, *d, None, None, a, a, q(*d, 3) - 4, 3, None) == WORKSPACE
    assert f(a, a, a, a, *d, a, a, a, a, q(*d, 3), 0, None) == WORKSPACE  # sized for a capped grid, called without the cap


def c16(B=1, L=2, H=4, W=5, G=2):
    t = torch.zeros(B, L, G, H, W, 16)
    t.lw = W
    return t


def test_python_refusals_without_gpu():
    x0, x1 = c16(H=2, W=3, G=4), c16()
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_block.convup_wgrad(x0, x1, x1, x1)
    with pytest.raises(ValueError, match="want"):
        last_block.convup_wgrad(x0, x1, x1, x1, want=())
    with pytest.raises(ValueError, match="want"):
        last_block.convup_wgrad(x0, x1, x1, x1, want=("weight", "bias"))
    with pytest.raises(ValueError, match="want"):
        last_block.convup_wgrad(x0, x1, x1, x1, want=("short", "short"))
    with pytest.raises(ValueError, match="max_workgroups"):
        last_block.convup_wgrad(x0, x1, x1, x1, max_workgroups=-1)
    with pytest.raises(ValueError, match="needs g1"):
        last_block.convup_wgrad(x0, x1, None, x1)
    with pytest.raises(ValueError, match="need gd"):
        last_block.convup_wgrad(x0, x1, x1, None, want=("weight", "short_bias"))
    assert last_block.WANT == ("weight", "short", "short_bias")
    with pytest.raises(ValueError, match="from_model"):
        last_block.TailConvs()(x0, x1)
    layer = last_block.TailConvs()
    assert [n for n, _ in layer.named_parameters()] == ["weight_bar", "short_weight", "short_bias"]
    assert all(p.requires_grad for p in layer.parameters())
    assert layer.weight_bar.shape == (32, 96, 3, 3, 3) and layer.short_weight.shape == (32, 96, 1, 1, 1)
    assert layer.weight_u.shape == (32,) and layer.weight_v.shape == (2592,)
    assert [n for n, _ in last_block.TailConvs(bias=False).named_parameters()] == ["weight_bar", "short_weight"]
    assert {n for n, _ in layer.named_buffers()} >= {"bn1_mean", "bn1_var", "bnd_mean", "bnd_var", "eps", "guard"}


def test_groups_parser_and_argument_checks_of_fit_last_block():
    assert finetune.LAST_BLOCK_GROUPS == finetune.TAIL_NORM_GROUPS + ("conv1", "convd")
    assert finetune.LAST_BLOCK_GROUPS == ("pred", "conv2", "bn2", "bn1", "bnd", "conv1", "convd")
    for bad in ((), ("pred", "conv3"), ("conv1", "conv1")):
        with pytest.raises(ValueError, match="train"):
            finetune.fit_last_block(None, None, None, train=bad, steps=1, lr=1e-3)
    x, g = torch.zeros(1, 2, 2, 4, 4), torch.zeros(1, 2, 20, 4, 4)
    with pytest.raises(ValueError, match="optimizer"):
        finetune.fit_last_block(None, x, g, train=("conv1",), steps=1, lr=1e-3, optimizer="lbfgs")
    with pytest.raises(ValueError, match="steps"):
        finetune.fit_last_block(None, x, g, train=("convd",), steps=-1, lr=1e-3)
    with pytest.raises(ValueError, match="windows"):
        finetune.fit_last_block(None, [x, x], [g], train=("conv1",), steps=1, lr=1e-3)
    parse = finetune.build_parser().parse_args
    assert parse(["--gt_events", "e.npz"]).train == "head"
    assert parse(["--gt_events", "e.npz", "--train", "last_block"]).train == "last_block"
    for old in ("head", "tail", "tail_norms"):
        assert parse(["--gt_events", "e.npz", "--train", old]).train == old


def test_effective_weight_follows_the_reference_iteration():
    z = load("b2_l3_5x7")
    layer = last_block.TailConvs()
    with torch.no_grad():
        for name, key in (("weight_bar", "weight_bar1"), ("weight_u", "u1"), ("weight_v", "v1")):
            getattr(layer, name).copy_(torch.from_numpy(z[key]))
    W = layer.effective()
    assert W.requires_grad
    assert np.abs(layer.weight_u.numpy() - z["ref32_u1_after"]).max() <= 1e-6
    assert np.abs(layer.weight_v.numpy() - z["ref32_v1_after"]).max() <= 1e-6
    f = R.block_forward(z["x0"], z["x1"], {k: z[k] for k in R.PARAMS})
    assert np.abs(W.detach().numpy() - f["W1"]).max() <= 1e-6 * np.abs(f["W1"]).max()
    # torch's autograd through sigma gives the closed form of the restatement
    g = R.block_grads(z["x0"], z["x1"], {k: z[k] for k in R.PARAMS}, z["upstream"], f)
    W.backward(torch.from_numpy(g["dW1"]).float())
    want = z["ref64_d_weight_bar1"]
    assert np.abs(layer.weight_bar.grad.numpy() - want).max() <= 2e-5 * np.abs(want).max()


def test_from_model_and_write_back_touch_the_two_convolutions_only():
    from v2ce_toolbox_amd import synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    layer = last_block.TailConvs.from_model(m)
    blk = m.UNet.decoders[-1]
    inner, short = blk.conv1.module, blk.downsample[0]
    assert torch.equal(layer.weight_bar.detach(), inner.weight_bar) and torch.equal(layer.weight_u, inner.weight_u)
    assert torch.equal(layer.short_weight.detach(), short.weight) and torch.equal(layer.short_bias.detach(), short.bias)
    assert torch.equal(layer.bn1_var, blk.bn1.running_var) and torch.equal(layer.bnd_mean, blk.downsample[1].running_mean)
    with torch.no_grad():
        layer.weight_bar.add_(1.0)
        layer.short_weight.sub_(2.0)
        layer.short_bias.add_(0.5)
        layer.weight_v.mul_(0.5)
    m._prep = {"stale": True}
    layer.write_back(m)
    assert m._prep is None
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    pre = "UNet.decoders.3."
    assert changed == {pre + "conv1.module.weight_bar", pre + "conv1.module.weight_v", pre + "downsample.0.weight",
                       pre + "downsample.0.bias"}
    assert not inner.weight_bar.requires_grad
    x0 = torch.zeros(1, 2, 4, 2, 3, 16, requires_grad=True)
    x0.lw = 3
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):        # (the device check comes first without a GPU)
        layer(x0, c16())
