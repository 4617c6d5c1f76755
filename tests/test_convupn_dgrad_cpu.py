"""CPU side of the tests of v2ce_convupn_dgrad (include/v2ce_hip_convupndgrad.h, tests/test_gpu_convupndgrad.py) and of the
layers built on it (dec2_block.Dec2ConvsThrough / Dec2BlockThrough): the header's symbols, the host-only size query and the
refusals that come before any device is touched, the numpy restatement of tests/convupn_dgrad_ref.py against torch's f64
autograd on the materialised upsample + concat, the exactness margin of the integer data of the GPU file's bit-for-bit
check, and what the new layer classes are without a model."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import convupn_dgrad_ref as R
from v2ce_toolbox_amd import conv_grads, dec2_block, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "v2ce_hip_convupndgrad.h"
BAD_ARG, WORKSPACE = -1, -4


def declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_the_symbols_of_the_convupndgrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVUPNDGRAD_EXPORTS) and len(set(hip.CONVUPNDGRAD_EXPORTS)) == 2
    older = (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS, hip.CONVUPGRAD_EXPORTS,
             hip.CONVUPDGRAD_EXPORTS, hip.CONVNGRAD_EXPORTS, hip.CONVUPNGRAD_EXPORTS)
    for other in older:
        assert not set(hip.CONVUPNDGRAD_EXPORTS) & set(other)
    # no other header names them, and this one names the older entries by file only (their own tests look for their symbols
    # in every other header)
    for other in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(other) != HEADER:
            assert not any(s in open(other).read() for s in syms), other
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    assert not any(s in own for o in older[3:] for s in o)
    m = re.search(r"#define\s+V2CE_UPNDGRAD_TERMS\(cout\)\s+\(28 \* \(cout\)\)", own)
    assert m and hip.UPNDGRAD_TERMS(32) == hip.UPDGRAD_TERMS == R.terms(32) and hip.UPNDGRAD_TERMS(64) == 1792 == R.terms(64)
    make = open(os.path.join(ROOT, "v2ce-toolbox_amd", "csrc", "Makefile")).read()
    rule = make.split("convupdgrad.o: convupdgrad.hip")[1].split("\n")
    assert HEADER in rule[0] and "$(EXACT)" in rule[1]
    assert (R.C0S, R.C1S, R.COUTS) == (hip.CONVUPN_C0, hip.CONVUPN_C1, hip.CONVUPN_COUT) and len(R.TRIPLES) == 8


def test_size_query():
    L = hip.lib()
    q, q_old = L.v2ce_convupn_dgrad_workspace_bytes, L.v2ce_convup_dgrad_workspace_bytes
    for shape in ((1, 1, 1, 1), (1, 3, 20, 70)):
        B, Lq, H, W = shape
        d = (B, Lq, H, W, W + 3, (W + 1) // 2 + 5)
        for c0, c1, cout in R.TRIPLES:
            # the repacked weights [group][unit][co][ci], and nothing for the grid
            assert q(c0, c1, cout, *d, 0) == q(c0, c1, cout, *d, 7) == (28 * cout * (c0 + c1) * 4 + 255) // 256 * 256 > 0
        assert q(*R.OLD, *d, 0) == q_old(*d, 0) and q(*R.OLD, *d, 3) == q_old(*d, 3)
        for c0 in (32, 96, 256):
            assert q(c0, 64, 64, *d, 0) == 0, c0
        for c in (16, 128):
            assert q(128, c, 64, *d, 0) == 0 and q(128, 64, c, *d, 0) == 0, c
    ok = R.DEC2
    assert q(*ok, 2, 3, 5, 7, 6, 4, 0) == 0                              # pitch < W
    assert q(*ok, 2, 3, 5, 7, 7, 3, 0) == 0 and q(*ok, 2, 3, 5, 8, 8, 4, 0) > 0      # pitch0 < W0 = (W + 1) / 2
    assert q(*ok, 2, 3, 5, 7, 7, 4, -1) == 0
    assert q(*ok, 0, 3, 5, 7, 7, 4, 0) == 0 and q(*ok, 2, 0, 5, 7, 7, 4, 0) == 0 and q(*ok, 2, 3, 0, 7, 7, 4, 0) == 0
    assert q(*ok, 2, 3, 5, 0, 7, 4, 0) == 0
    assert q(*ok, 4096, 4096, 16, 16, 16, 8, 0) == 0                     # 2^32 positions
    assert q(*ok, 1, 1 << 20, 1, 1 << 10, 1 << 14, 1 << 9, 0) == 0       # B L H pitch = 2^34
    assert q(*ok, 1, 1 << 20, 1, 1 << 10, 1 << 10, 1 << 14, 0) == 0      # B L H0 pitch0 = 2^34


def test_argument_validation_without_gpu():
    """Every refusal the header lists comes back before a device is touched (the addresses below are never dereferenced)."""
    L = hip.lib()
    q, f = L.v2ce_convupn_dgrad_workspace_bytes, L.v2ce_convupn_dgrad
    a, big = 4096, 1 << 30                                              # aligned stand-ins for device addresses
    d = (2, 3, 5, 7, 7, 4)
    ok = R.DEC2
    for tr in ((32, 64, 64), (96, 64, 64), (256, 64, 64), (128, 16, 64), (128, 128, 64), (128, 64, 16), (128, 64, 128), (0, 32, 32),
               (64, 33, 32), (-64, 32, 32)):
        assert f(a, a, a, a, *tr, *d, a, a, a, big, 0, None) == BAD_ARG, tr
        assert b"c0" in L.v2ce_last_error()
    for dims in ((0, 3, 5, 7, 7, 4), (2, 0, 5, 7, 7, 4), (2, 3, 0, 7, 7, 4), (2, 3, 5, 0, 7, 4)):
        assert f(a, a, a, a, *ok, *dims, a, a, a, big, 0, None) == BAD_ARG, dims
    assert f(a, a, a, a, *ok, 2, 3, 5, 7, 6, 4, a, a, a, big, 0, None) == BAD_ARG and b"pitch" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, 2, 3, 5, 7, 7, 3, a, a, a, big, 0, None) == BAD_ARG and b"pitch0" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, *d, a, a, a, big, -1, None) == BAD_ARG and b"max_workgroups" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, 4096, 4096, 16, 16, 16, 8, a, a, a, big, 0, None) == BAD_ARG
    assert f(a, a, a, a, *ok, 1, 1 << 20, 1, 1 << 10, 1 << 14, 1 << 9, a, a, a, big, 0, None) == BAD_ARG
    assert f(a, a, a, a, *ok, 1, 1 << 20, 1, 1 << 10, 1 << 10, 1 << 14, a, a, a, big, 0, None) == BAD_ARG
    assert f(a, a, None, None, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()       # g1 and gd
    assert f(None, a, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()          # g1 needs weight
    assert f(a, None, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()          # gd needs short_weight
    assert f(a, a, a, a, *ok, *d, None, None, a, big, 0, None) == BAD_ARG and b"no output" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, *d, a, a, None, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()          # no workspace
    for bad in ((a + 4, a, a, a), (a, a + 8, a, a), (a, a, a + 4, a), (a, a, a, a + 12)):                          # g1, gd, d_x0, d_x1
        assert f(a, a, bad[0], bad[1], *ok, *d, bad[2], bad[3], a, big, 0, None) == BAD_ARG and b"16-byte" in L.v2ce_last_error()
    for w, s in ((a + 2, a), (a, a + 1)):
        assert f(w, s, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"4-byte" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, *d, a, a, a + 4, big, 0, None) == BAD_ARG and b"8-byte" in L.v2ce_last_error()
    for tr in R.TRIPLES:
        need = q(*tr, *d, 0)
        assert f(a, a, a, a, *tr, *d, a, a, a, need - 4, 0, None) == WORKSPACE and b"workspace too small" in L.v2ce_last_error()
    # what nothing needs may be NULL, and a weight at 4 bytes is fine: these get as far as the workspace check
    need = q(*ok, *d, 3)
    assert f(None, a, None, a, *ok, *d, a, a, a, need - 4, 3, None) == WORKSPACE     # the shortcut's share alone
    assert f(a, None, a, None, *ok, *d, a, a, a, need - 4, 3, None) == WORKSPACE     # conv1's share alone
    assert f(a + 4, a + 12, a, a, *ok, *d, None, a, a, need - 4, 0, None) == WORKSPACE   # d_x1 alone
    assert f(a, a, a, a, *ok, *d, a, None, a, need - 4, 0, None) == WORKSPACE        # d_x0 alone
    assert b"v2ce_convupn_dgrad" in L.v2ce_last_error()                  # the message leads with the entry that was called
    assert L.v2ce_convup_dgrad(a, a, a, a, *d, a, None, a, 4, 0, None) == WORKSPACE and b"v2ce_convup_dgrad" in L.v2ce_last_error()


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 4, 65)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c0,c1,cout", [R.DEC2, R.OLD, (128, 32, 64)])
def test_restatement_matches_torch_f64_autograd(c0, c1, cout, shape):
    """conv3d + 1x1x1 conv3d on cat(interpolate(x0, size=(L, H, W), mode='nearest'), x1), CPU, double: the gradients of
    <g1, conv1> + <gd, shortcut> with respect to x0 and x1, to 1e-12 relative to an element's sum of |terms|."""
    z, t = R.inputs(shape, c0, c1, cout), R.truth(shape, c0, c1, cout)
    B, L, H, W = shape
    x0 = torch.zeros(B, c0, L, (H + 1) // 2, (W + 1) // 2, dtype=torch.float64, requires_grad=True)
    x1 = torch.zeros(B, c1, L, H, W, dtype=torch.float64, requires_grad=True)
    X = torch.cat([torch.nn.functional.interpolate(x0, size=(L, H, W), mode="nearest"), x1], dim=1)
    kw, ks = torch.from_numpy(z["kw"].copy()).double(), torch.from_numpy(z["ks"].copy()).double()
    y1 = torch.nn.functional.conv3d(X, kw, padding=1)
    yd = torch.nn.functional.conv3d(X, ks.view(cout, c0 + c1, 1, 1, 1))
    ((y1 * torch.from_numpy(z["g1"].copy()).double()).sum() + (yd * torch.from_numpy(z["gd"].copy()).double()).sum()).backward()
    for k, g in (("x0", x0.grad), ("x1", x1.grad)):
        want, S = t[f"d_{k}"], t[f"abs_{k}"]
        assert tuple(g.shape) == want.shape and S.min() >= 0 and S.max() > 0
        assert np.all(np.abs(g.numpy() - want) <= 1e-12 * S), k
        assert np.all(np.abs(want) <= S)
    assert t["n_x0"].sum() == H * W and t["n_x0"].shape == ((H + 1) // 2, (W + 1) // 2)
    if shape == (1, 2, 4, 65):
        assert np.array_equal(t["n_x0"][:, 32], [2, 2]) and np.all(t["n_x0"][:, :32] == 4)
        assert np.array_equal(t["d_x0"][..., 32], t["d_X"][:, :c0, :, 0::2, 64] + t["d_X"][:, :c0, :, 1::2, 64])


def test_the_shares_of_the_restatement_add_up():
    z, both = R.inputs((2, 3, 5, 7), *R.DEC2), R.truth((2, 3, 5, 7), *R.DEC2)
    conv, short = R.dgrad(*R.DEC2, z["kw"], None, z["g1"], None), R.dgrad(*R.DEC2, None, z["ks"], None, z["gd"])
    for k in ("d_x0", "d_x1", "abs_x0", "abs_x1"):
        assert np.abs(conv[k] + short[k] - both[k]).max() <= 1e-13 * np.abs(both[k]).max(), k


def test_integer_data_of_the_bit_for_bit_check_is_exact_in_f32():
    """With |g| <= 8 and |w| <= 4 a product is at most 32 in magnitude, and a d_x0 element at cout = 64 sums at most 4
    positions x 28 units x 64 output channels of them: every partial sum, in any order, is an integer below 2^24, hence an
    f32, so the kernel's sums and the f64 truth agree to the bit."""
    assert (R.G_TOP, R.W_TOP) == (8, 4)
    most = 4 * hip.UPNDGRAD_TERMS(64) * R.G_TOP * R.W_TOP
    assert most == 4 * 28 * 64 * 32 == 229376 < 2 ** 24
    for tr in (R.DEC2, (128, 32, 64)):
        z, t = R.inputs((2, 3, 5, 7), *tr, "int", 5), R.truth((2, 3, 5, 7), *tr, "int", 5)
        assert np.abs(z["g1"]).max() == R.G_TOP and np.abs(z["kw"]).max() == R.W_TOP
        for k in ("d_x0", "d_x1", "abs_x0", "abs_x1"):
            assert np.array_equal(t[k], np.round(t[k])) and 0 < np.abs(t[k]).max() <= most, k
        assert np.array_equal(t["d_x0"].astype(np.float32).astype(np.float64), t["d_x0"])


def test_through_layers_without_a_model():
    convs, through = dec2_block.Dec2Convs(), dec2_block.Dec2ConvsThrough(input_grads=True)
    assert through.input_grads is True and dec2_block.Dec2ConvsThrough().input_grads is False
    assert dec2_block.Dec2ConvsThrough.DGRAD is True and dec2_block.Dec2Convs.DGRAD is False
    assert issubclass(dec2_block.Dec2ConvsThrough, dec2_block.Dec2Convs)
    assert list(through.state_dict()) == list(convs.state_dict())
    assert [(n, tuple(p.shape)) for n, p in through.named_parameters()] == [(n, tuple(p.shape)) for n, p in convs.named_parameters()]
    with pytest.raises(ValueError, match="no gradient with respect to x0 and x1"):
        dec2_block.Dec2Convs(input_grads=True)
    assert "no gradient with respect to x0 and x1" in dec2_block.Dec2ConvsThrough.NO_INPUT_GRADS
    parts = lambda cls: cls(cls.CONVS(input_grads=cls.CONVS.DGRAD), cls.NORMS(), cls.CONV())
    block, plain = parts(dec2_block.Dec2BlockThrough), parts(dec2_block.Dec2Block)
    assert dec2_block.Dec2BlockThrough.CONVS is dec2_block.Dec2ConvsThrough and dec2_block.Dec2Block.CONVS is dec2_block.Dec2Convs
    assert (dec2_block.Dec2BlockThrough.NORMS, dec2_block.Dec2BlockThrough.CONV) == (dec2_block.Dec2Norms, dec2_block.Dec2Conv)
    assert block.convs.input_grads is True and plain.convs.input_grads is False
    assert list(block.state_dict()) == list(plain.state_dict()) and len(list(block.parameters())) == 10
    with torch.no_grad():
        block.convs.short_weight.add_(1.5)
    plain.load_state_dict(block.state_dict())
    block.load_state_dict(plain.state_dict())
    assert torch.equal(plain.convs.short_weight, block.convs.short_weight)
    assert dec2_block.DGRAD_WANT == ("x0", "x1") and dec2_block.convupn_dgrad is conv_grads.convupn_dgrad
    # the entry is looked up in the module when it is called
    assert through._dgrad is not dec2_block.convupn_dgrad


def c16(planes, B=1, L=2, H=4, W=5):
    t = torch.zeros(B, L, planes, H, W, 16)
    t.lw = W
    return t


def test_python_refusals_without_gpu():
    g = c16(4)
    w, s = torch.zeros(64, 192, 3, 3, 3), torch.zeros(64, 192)
    f = conv_grads.convupn_dgrad
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        f(w, s, g, g)
    with pytest.raises(ValueError, match="want"):
        f(w, s, g, g, want=())
    with pytest.raises(ValueError, match="want"):
        f(w, s, g, g, want=("x0", "x2"))
    with pytest.raises(ValueError, match="max_workgroups"):
        f(w, s, g, g, max_workgroups=-1)
    with pytest.raises(ValueError, match="both None"):
        f(w, s, None, None)
    with pytest.raises(ValueError, match="needs weight"):
        f(None, s, g, g)
    with pytest.raises(ValueError, match="needs short_weight"):
        f(w, None, g, g)
    # 128 input channels do not say how they split: refused before any device check, with both readings named
    w128, s128 = torch.zeros(64, 128, 3, 3, 3), torch.zeros(64, 128)
    with pytest.raises(ValueError, match=r"64 \+ 64 or as 128 \+ 0"):
        f(w128, s128, g, g)
    with pytest.raises(ValueError, match=r"64 \+ 64 or as 128 \+ 0"):
        f(None, s128, None, g)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):            # said: the call goes on to the device check
        f(w128, s128, g, g, c0=64)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        f(w128, s128, g, g, out={"x0": c16(4, H=2, W=3)})
    with pytest.raises(ValueError, match="does not split"):
        f(w128, s128, g, g, c0=128)
    with pytest.raises(ValueError, match="does not split"):
        f(w, s, g, g, c0=64)
