"""CPU side of the input gradients of the last decoder block's conv1 and shortcut (include/v2ce_hip_convupdgrad.h,
last_block.py: convup_dgrad, TailConvs(input_grads=True), LastBlock): the goldens' files, the numpy restatement
(tests/last_block_dgrad_ref.py) against torch's f64 conv3d input gradients and upsample backward
(tests/golden/.lastblock_dgrad/), the export tuple against its header, and what the C ABI and the Python layer refuse
without a GPU."""
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import last_block_dgrad_ref as D
from tests import last_block_ref as R
from tests.make_last_block_dgrad_goldens import CASES, KERNEL_ONLY, SIZE_CAP, file_names
from v2ce_toolbox_amd import hip, last_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "v2ce_hip_convupdgrad.h"
BAD_ARG, WORKSPACE = -1, -4
LAYER_CASES = [n for n in sorted(CASES) if n not in KERNEL_ONLY]

load = D.load_case


def test_goldens_are_the_recipes_files_and_small():
    files = sorted(glob.glob(os.path.join(D.GOLD, "*.npz")))
    assert sorted(os.path.basename(p) for p in files) == sorted(file_names())
    for p in files:
        assert os.path.getsize(p) <= SIZE_CAP, p
    assert set(CASES) == {"b1_l1_1x1", "b2_l3_5x7", "b1_l2_3x70", "b1_l3_6x64", "zero", "b1_l3_20x70", "b1_l2_4x65"}
    assert CASES["b1_l2_4x65"] == (1, 2, 4, 65) and "b1_l2_4x65" in KERNEL_ONLY and len(LAYER_CASES) == 5
    for name, (B, L, H, W) in CASES.items():
        z = load(name)
        x0, x1 = (B, 64, L, (H + 1) // 2, (W + 1) // 2), (B, 32, L, H, W)
        assert z["kw"].shape == (32, 96, 3, 3, 3) and z["ks"].shape == (32, 96) and z["kw"].dtype == z["ks"].dtype == np.float32
        assert np.array_equal(z["kw"] * 64, np.round(z["kw"] * 64)) and np.array_equal(z["ks"] * 64, np.round(z["ks"] * 64))
        assert z["g1"].shape == z["gd"].shape == x1 and z["g1"].dtype == z["gd"].dtype == np.float32, name
        assert z["ref64_d_x0"].shape == z["abs_terms_d_x0"].shape == x0 and z["ref64_d_x1"].shape == z["abs_terms_d_x1"].shape == x1
        assert all(z[k].dtype == np.float64 for k in z if k.startswith(("ref64", "abs_terms", "ref32_dev"))), name
        if name not in KERNEL_ONLY:
            assert z["ref64_layer_d_x0"].shape == x0 and z["ref64_layer_d_x1"].shape == x1
            assert float(z["ref32_dev_layer_d_x0"]) >= 0 and float(z["ref32_dev_layer_d_x1"]) >= 0
    z = load("b1_l3_20x70")
    assert float(z["ref32_dev_d_x0"]) > 0 and float(z["ref32_dev_d_x1"]) > 0      # f32 sums of its terms do round
    assert not load("zero")["ref64_d_x0"].any() and not load("zero")["ref64_layer_d_x1"].any()


def test_terms_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    m = re.search(r"#define\s+V2CE_UPDGRAD_TERMS\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.UPDGRAD_TERMS == 32 * 28


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_input_gradients_match_torch_f64(name):
    z = load(name)
    g = D.dgrad(z["kw"], z["ks"], z["g1"], z["gd"])
    for got, key in ((g["d_x0"], "ref64_d_x0"), (g["d_x1"], "ref64_d_x1"), (g["abs_x0"], "abs_terms_d_x0"),
                     (g["abs_x1"], "abs_terms_d_x1")):
        assert got.shape == z[key].shape
        assert np.abs(got - z[key]).max() <= 1e-12 * max(np.abs(z[key]).max(), 1e-300), key
    B, L, H, W = CASES[name]
    assert g["n_x0"].shape == ((H + 1) // 2, (W + 1) // 2) and g["n_x0"].sum() == H * W
    if name == "zero":
        assert not z["ref64_d_x0"].any() and not z["ref64_d_x1"].any()
    else:
        assert np.all(np.abs(g["d_x0"]) <= g["abs_x0"]) and np.all(np.abs(g["d_x1"]) <= g["abs_x1"])
    if name == "b1_l1_1x1":                          # only the centre tap and the shortcut see the single position
        centre = z["kw"].astype(np.float64)[:, :, 1, 1, 1]
        want = z["g1"].astype(np.float64).reshape(32) @ centre + z["gd"].astype(np.float64).reshape(32) @ z["ks"].astype(np.float64)
        assert np.abs(g["d_X"].reshape(96) - want).max() <= 1e-13 * np.abs(want).max()
        assert np.array_equal(g["d_x0"].reshape(64), g["d_X"].reshape(96)[:64]) and g["n_x0"].tolist() == [[1.0]]
    if name == "b2_l3_5x7":
        # the last source row (h0 = 2) is output row 4 alone and the last source column (w0 = 3) output column 6 alone
        dX = g["d_X"][:, :64]
        assert np.array_equal(g["d_x0"][:, :, :, 2, :3], dX[:, :, :, 4, 0:6:2] + dX[:, :, :, 4, 1:6:2])
        assert np.array_equal(g["d_x0"][:, :, :, :2, 3], dX[:, :, :, 0:4:2, 6] + dX[:, :, :, 1:4:2, 6])
        assert np.array_equal(g["d_x0"][:, :, :, 2, 3], dX[:, :, :, 4, 6])
        assert g["n_x0"].tolist() == [[4, 4, 4, 2], [4, 4, 4, 2], [2, 2, 2, 1]]
    if name == "b1_l2_4x65":
        assert np.array_equal(g["n_x0"][:, 32], [2, 2]) and np.all(g["n_x0"][:, :32] == 4)


def test_the_shares_of_the_restatement_add_up_and_the_bound_grows_with_n():
    z = load("b2_l3_5x7")
    both = D.dgrad(z["kw"], z["ks"], z["g1"], z["gd"])
    conv, short = D.dgrad(z["kw"], None, z["g1"], None), D.dgrad(None, z["ks"], None, z["gd"])
    for k in ("d_x0", "d_x1", "abs_x0", "abs_x1"):
        assert np.abs(conv[k] + short[k] - both[k]).max() <= 1e-13 * np.abs(both[k]).max(), k
    a = np.array([1.0, 2.0])
    assert np.array_equal(D.dgrad_bound(a, 896), 897 * 2.0 ** -24 * a + 896 * 2.0 ** -126)
    assert np.all(D.dgrad_bound(a, np.array([896, 4 * 896])) == [897 * 2.0 ** -24 + 896 * 2.0 ** -126,
                                                                   (4 * 896 + 1) * 2.0 ** -24 * 2 + 4 * 896 * 2.0 ** -126])


@pytest.mark.parametrize("name", LAYER_CASES)
def test_restated_block_gives_the_reference_blocks_input_gradients(name):
    z = load(name)
    p = {k: z[k] for k in R.PARAMS}
    f = R.block_forward(z["x0"], z["x1"], p)
    assert np.array_equal(z["mask_t"], f["pre1"] > 0) and np.array_equal(z["mask_y"], f["pre"] > 0)
    g = R.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    r = D.dgrad(f["rs1"][:, None, None, None, None] * f["W1"], f["rsd"][:, None] * z["short_weight"].astype(np.float64).reshape(32, 96),
                g["g1"], g["gd"])
    for k in ("x0", "x1"):
        want = z[f"ref64_layer_d_{k}"]
        assert np.abs(r[f"d_{k}"] - want).max() <= 1e-11 * max(np.abs(want).max(), 1e-300), k
    if name != "zero":
        assert np.abs(z["ref64_layer_d_x0"]).max() > 0 and np.abs(z["ref64_layer_d_x1"]).max() > 0


def declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_symbols_of_the_convupdgrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVUPDGRAD_EXPORTS) and len(set(hip.CONVUPDGRAD_EXPORTS)) == len(hip.CONVUPDGRAD_EXPORTS)
    older = (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS, hip.CONVUPGRAD_EXPORTS)
    for other in older:
        assert not set(hip.CONVUPDGRAD_EXPORTS) & set(other)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != HEADER]
    assert len(others) >= 6
    for other in others:
        assert not any(s in open(other).read() for s in syms), other
    # the header names the older entries by file only (their own tests look for their symbols in every other header)
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    assert not any(s in own for s in hip.CONVGRAD_EXPORTS + hip.CONVDGRAD_EXPORTS + hip.CONVUPGRAD_EXPORTS)


def test_size_queries_and_refusals_without_gpu():
    L = hip.lib()
    q, f = L.v2ce_convup_dgrad_workspace_bytes, L.v2ce_convup_dgrad
    packed = 3 * 28 * 32 * 32 * 4                                       # the repacked weights: [group][unit][co][ci] f32
    assert packed % 256 == 0
    assert q(1, 1, 1, 1, 1, 1, 0) == q(2, 3, 5, 7, 7, 4, 0) == q(1, 3, 20, 70, 96, 35, 7) == packed
    assert q(4, 16, 260, 346, 352, 173, 0) == q(1, 16, 260, 346, 352, 192, 1000) == packed      # the grid needs nothing
    assert q(0, 3, 5, 7, 7, 4, 0) == 0 and q(2, 0, 5, 7, 7, 4, 0) == 0 and q(2, 3, 0, 7, 7, 4, 0) == 0 and q(2, 3, 5, 0, 7, 4, 0) == 0
    assert q(2, 3, 5, 7, 6, 4, 0) == 0                                  # pitch < W
    assert q(2, 3, 5, 7, 7, 3, 0) == 0 and q(2, 3, 5, 8, 8, 4, 0) > 0   # pitch0 < W0 = (W + 1) / 2
    assert q(2, 3, 5, 7, 7, 4, -1) == 0
    assert q(4096, 4096, 16, 16, 16, 8, 0) == 0                         # 2^32 positions
    assert q(1, 1 << 20, 1, 1 << 10, 1 << 14, 1 << 9, 0) == 0 and q(1, 1 << 20, 1, 1 << 10, 1 << 10, 1 << 14, 0) == 0   # a pitch
    d = (2, 3, 5, 7, 7, 4)
    a = 4096                                                            # aligned stand-ins for device addresses
    big = 1 << 30
    # refused before anything is launched (the addresses below are never dereferenced)
    assert f(a, a, None, None, *d, a, a, a, big, 0, None) == BAD_ARG    # g1 and gd both NULL
    assert b"null" in L.v2ce_last_error()
    assert f(a, a, a, a, 2, 3, 5, 7, 6, 4, a, a, a, big, 0, None) == BAD_ARG
    assert b"pitch" in L.v2ce_last_error()
    assert f(a, a, a, a, 2, 3, 5, 7, 7, 3, a, a, a, big, 0, None) == BAD_ARG
    assert b"pitch0" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, None, None, a, big, 0, None) == BAD_ARG
    assert b"no output" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a, big, -1, None) == BAD_ARG
    assert f(a, a, a, a, *d, a, a, None, big, 0, None) == BAD_ARG       # no workspace
    assert f(None, a, a, a, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()    # g1 needs weight
    assert f(a, None, a, a, *d, a, a, a, big, 0, None) == BAD_ARG       # gd needs short_weight
    for bad in ((a + 4, a, a, a), (a, a + 8, a, a), (a, a, a + 4, a), (a, a, a, a + 12)):               # g1, gd, d_x0, d_x1
        assert f(a, a, bad[0], bad[1], *d, bad[2], bad[3], a, big, 0, None) == BAD_ARG
        assert b"16-byte" in L.v2ce_last_error()
    for w, s in ((a + 2, a), (a, a + 1)):
        assert f(w, s, a, a, *d, a, a, a, big, 0, None) == BAD_ARG
        assert b"4-byte" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a + 4, big, 0, None) == BAD_ARG
    assert b"8-byte" in L.v2ce_last_error()
    assert f(a, a, a, a, *d, a, a, a, q(*d, 0) - 4, 0, None) == WORKSPACE
    # what nothing needs may be NULL, and a weight at 4 bytes is fine: these get as far as the workspace check
    assert f(None, a, None, a, *d, a, a, a, q(*d, 3) - 4, 3, None) == WORKSPACE     # the shortcut's share alone
    assert f(a, None, a, None, *d, a, a, a, q(*d, 3) - 4, 3, None) == WORKSPACE     # conv1's share alone
    assert f(a + 4, a + 12, a, a, *d, None, a, a, q(*d, 0) - 4, 0, None) == WORKSPACE   # d_x1 alone
    assert f(a, a, a, a, *d, a, None, a, q(*d, 0) - 4, 0, None) == WORKSPACE        # d_x0 alone


def c16(B=1, L=2, H=4, W=5, G=2):
    t = torch.zeros(B, L, G, H, W, 16)
    t.lw = W
    return t


def test_python_refusals_without_gpu():
    w, s, g = torch.zeros(32, 96, 3, 3, 3), torch.zeros(32, 96), c16()
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        last_block.convup_dgrad(w, s, g, g)
    with pytest.raises(ValueError, match="want"):
        last_block.convup_dgrad(w, s, g, g, want=())
    with pytest.raises(ValueError, match="want"):
        last_block.convup_dgrad(w, s, g, g, want=("x0", "x2"))
    with pytest.raises(ValueError, match="want"):
        last_block.convup_dgrad(w, s, g, g, want=("x1", "x1"))
    with pytest.raises(ValueError, match="max_workgroups"):
        last_block.convup_dgrad(w, s, g, g, max_workgroups=-1)
    with pytest.raises(ValueError, match="both None"):
        last_block.convup_dgrad(w, s, None, None)
    with pytest.raises(ValueError, match="needs weight"):
        last_block.convup_dgrad(None, s, g, g)
    with pytest.raises(ValueError, match="needs short_weight"):
        last_block.convup_dgrad(w, None, g, g)
    assert last_block.DGRAD_WANT == ("x0", "x1")
    assert inspect.signature(last_block.convup_dgrad).parameters["want"].default == ("x0", "x1")


def test_tail_convs_defaults_to_no_input_grads_and_last_block_composes_the_three_layers():
    from v2ce_toolbox_amd import last_conv, synth
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    assert last_block.TailConvs().input_grads is False and last_block.TailConvs(input_grads=True).input_grads is True
    assert inspect.signature(last_block.TailConvs.__init__).parameters["input_grads"].default is False
    assert inspect.signature(last_block.TailConvs.from_model).parameters["input_grads"].default is False
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    assert last_block.TailConvs.from_model(m).input_grads is False
    assert last_block.TailConvs.from_model(m, input_grads=True).input_grads is True
    block = last_block.LastBlock.from_model(m)
    assert isinstance(block.convs, last_block.TailConvs) and block.convs.input_grads is True
    assert isinstance(block.norms, last_conv.TailNorms) and isinstance(block.conv, last_conv.LastConv)
    assert len(list(block.parameters())) == 10 and all(p.requires_grad for p in block.parameters())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        block.convs.short_weight.sub_(2.0)
        block.norms.bn1_bias.add_(0.5)
        block.conv.bn_weight.mul_(0.5)
    m._prep = {"stale": True}
    block.write_back(m)
    assert m._prep is None
    after = m.state_dict()
    pre = "UNet.decoders.3."
    assert {k for k in before if not torch.equal(before[k], after[k])} == {pre + "downsample.0.weight", pre + "bn1.bias", pre + "bn2.weight"}
    # the default layer still refuses sources that require grad; both forms refuse the CPU first
    x0 = torch.zeros(1, 2, 4, 2, 3, 16, requires_grad=True)
    x0.lw = 3
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        block(x0, c16())
