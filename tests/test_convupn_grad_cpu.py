"""CPU side of the tests of v2ce_convupn_wgrad (include/v2ce_hip_convupngrad.h, tests/test_gpu_convupngrad.py) and of the
dec2 block built on it: the truths of tests/convupn_ref.py against torch.nn.grad in f64 on the materialised upsample + concat,
the header's symbols and the Makefile's lines, the share arithmetic and the refusals from the host-only size query, the
exactness margin of the integer data of check A, the command line's choices, and the goldens of tests/golden/.dec2block
against their recipe's restatement (tests/dec2_block_ref.py)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import convupn_ref as R
from tests import dec2_block_ref as B2
from tests import grad_walk_ref as G
from tests.make_last_block_dgrad_goldens import SIZE_CAP
from v2ce_toolbox_amd import finetune, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "v2ce_hip_convupngrad.h"
BAD_ARG, WORKSPACE = -1, -4
ALL = R.TRIPLES + (R.OLD,)
PARTIAL = (28 * 32 * 32 + 32) * 8                                    # f64 bytes of one workgroup's partial sums
SMALL_SHAPES = [s for s in R.SMALL if s != (1, 3, 20, 70)]


def dims(shape, pitch0=None):
    B, L, H, W = shape
    return (B, L, H, W, G.pitch_of(W), G.pitch_of((W + 1) // 2) if pitch0 is None else pitch0)


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c0,c1,cout", ALL)
def test_truths_match_numpy_and_torch_nn_grad(c0, c1, cout, shape):
    """Three statements of the same f64 sums: the device truth of the GPU tests (one matmul per tap on the gathered source),
    the numpy restatement of the header's formulas (term by term), and torch.nn.grad.conv3d_weight on
    cat(F.interpolate(x0, size, mode='nearest'), x1) -- the 3x3x3 weight with g1, the 1x1x1 weight and the bias with gd.  Each
    is within n 2^-53 S of the exact sum of an element's n terms, so two of them differ by at most n 2^-52 S."""
    z = R.inputs(shape, c0, c1, cout, False, 17)
    t = R.wgrad_truth(z["x0"], z["x1"], z["g1"], z["gd"])
    n_ = R.wgrad_np(z["x0"].numpy(), z["x1"].numpy(), z["g1"].numpy(), z["gd"].numpy())
    L, H, W = shape[1:]
    up = torch.nn.functional.interpolate(z["x0"].double(), size=(L, H, W), mode="nearest")
    X = torch.cat([up, z["x1"].double()], dim=1)
    assert torch.equal(X, R.virtual_input(z["x0"].double(), z["x1"].double()))
    ref_w = torch.nn.grad.conv3d_weight(X, (cout, c0 + c1, 3, 3, 3), z["g1"].double(), padding=1)
    ref_s = torch.nn.grad.conv3d_weight(X, (cout, c0 + c1, 1, 1, 1), z["gd"].double()).reshape(cout, c0 + c1)
    ref_b = z["gd"].double().sum(dim=(0, 2, 3, 4))
    n = int(np.prod(shape))
    assert tuple(t["d_weight"].shape) == (cout, c0 + c1, 3, 3, 3) and tuple(t["d_short"].shape) == (cout, c0 + c1)
    for key, ab, others in (("d_weight", "abs_weight", (n_["d_weight"], ref_w.numpy())), ("d_short", "abs_short", (n_["d_short"], ref_s.numpy())),
                            ("d_short_bias", "abs_short_bias", (n_["d_short_bias"], ref_b.numpy()))):
        tol = n * 2.0 ** -52 * t[ab].numpy()
        assert t[ab].min() >= 0 and t[ab].max() > 0
        for other in others:
            assert other.shape == tuple(t[key].shape) and np.all(np.abs(t[key].numpy() - other) <= tol), key


def declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_symbols_of_the_convupngrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVUPNGRAD_EXPORTS) and len(set(hip.CONVUPNGRAD_EXPORTS)) == len(hip.CONVUPNGRAD_EXPORTS)
    older = (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS, hip.CONVUPGRAD_EXPORTS,
             hip.CONVUPDGRAD_EXPORTS, hip.CONVNGRAD_EXPORTS)
    for other in older:
        assert not set(hip.CONVUPNGRAD_EXPORTS) & set(other)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != HEADER]
    assert len(others) >= 8
    for other in others:
        assert not any(s in open(other).read() for s in syms), other
    # the header names the older entries by file only (their own tests look for their symbols in every other header)
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    assert not any(s in own for s in hip.CONVGRAD_EXPORTS + hip.CONVDGRAD_EXPORTS + hip.CONVUPGRAD_EXPORTS + hip.CONVUPDGRAD_EXPORTS +
                   hip.CONVNGRAD_EXPORTS)
    make = open(os.path.join(ROOT, "v2ce-toolbox_amd", "csrc", "Makefile")).read()
    links = [ln for ln in make.splitlines() if "-shared" in ln]
    assert len(links) >= 6 and all("convupnwgrad.o" in ln or "$(OBJS)" in ln for ln in links)
    assert "convupnwgrad.o" in [ln for ln in make.splitlines() if ln.startswith("OBJS")][0]
    rule = make.split("convupnwgrad.o: convupnwgrad.hip")[1].split("\n")[1]
    assert "$(EXACT)" in rule
    assert hip.UPWGRAD_CHAIN == 4096 and "V2CE_UPWGRAD_CHAIN" in own


def test_size_query_follows_the_documented_shares_and_equals_the_older_entrys():
    L = hip.lib()
    q, q_old = L.v2ce_convupn_wgrad_workspace_bytes, L.v2ce_convup_wgrad_workspace_bytes
    up256 = lambda n: (n + 255) // 256 * 256
    shapes = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 3, 20, 70), (1, 16, 130, 173), (1, 16, 260, 346), R.WALK]
    for c0, c1, cout in ALL:
        p = R.pairs_of(c0, c1, cout)
        for s in shapes:
            d, tiles = dims(s), G.conv_tiles(*s)
            for cap in (0, 1, 2, 3, 4, 5, 8, 12, 13, 97, 255, 256, 1000):
                assert q(c0, c1, cout, *d, cap) == up256(R.shares(c0, c1, cout, tiles, cap) * p * PARTIAL), (c0, c1, cout, d, cap)
                if (c0, c1, cout) == R.OLD:
                    assert q(c0, c1, cout, *d, cap) == q_old(*d, cap), (d, cap)
    assert R.pairs_of(128, 64, 64) == 12 and R.pairs_of(*R.OLD) == 3 and R.shares(*R.OLD, 10 ** 6) == 85
    # dec2's shape: 3120 tiles over 21 shares on 252 workgroups
    assert G.conv_tiles(1, 16, 130, 173) == 3120 and R.shares(128, 64, 64, 3120) == 21
    assert q(128, 64, 64, 1, 16, 130, 173, 192, 96, 0) == up256(252 * PARTIAL)


def test_walk_shape_puts_the_default_grid_at_its_cap_on_uneven_shares():
    B, Lq, H, W = R.WALK
    q = hip.lib().v2ce_convupn_wgrad_workspace_bytes
    d = dims(R.WALK)
    tiles = G.conv_tiles(*R.WALK)
    assert tiles == 396 and d[4] > W and H % 2 == 1 and W % 64 == 3      # a one-row last tile row, a three-column last tile
    for c0, c1, cout in R.TRIPLES:
        p = R.pairs_of(c0, c1, cout)
        cap = R.CAP // p
        assert tiles > cap and tiles % cap != 0 and R.shares(c0, c1, cout, tiles) == cap
        assert q(c0, c1, cout, *d, 0) == q(c0, c1, cout, *d, R.CAP) == q(c0, c1, cout, *d, 10 ** 6) == cap * p * PARTIAL
        assert q(c0, c1, cout, *d, 0) > q(c0, c1, cout, *d, (cap - 1) * p) > 0
        prime = R.shares(c0, c1, cout, tiles, R.PRIME_GRID)
        assert prime == max(R.PRIME_GRID // p, 1) and q(c0, c1, cout, *d, R.PRIME_GRID) == (prime * p * PARTIAL + 255) // 256 * 256
        sizes = G.share_sizes(tiles, cap)
        assert sum(sizes) == tiles and tiles % cap != 0 and max(sizes) == min(sizes) + 1 and min(sizes) >= 1, (c0, c1, cout)
        assert sum(G.share_sizes(tiles, prime)) == tiles and 1 <= prime < cap
    # the one-share row of the small shapes: 60 tiles, a full chain of 32 tiles and a partial one of 28
    shape = (1, 3, 20, 70)
    assert R.SMALL[shape] == 1 and G.conv_tiles(*shape) == 60 and hip.UPWGRAD_CHAIN // 128 == 32
    for c0, c1, cout in R.TRIPLES:
        p = R.pairs_of(c0, c1, cout)
        assert R.shares(c0, c1, cout, 60, p) == 1 and q(c0, c1, cout, *dims(shape), p) == (p * PARTIAL + 255) // 256 * 256


def test_refusals_without_gpu():
    L = hip.lib()
    q, f = L.v2ce_convupn_wgrad_workspace_bytes, L.v2ce_convupn_wgrad
    a, big = 4096, 1 << 30                                              # aligned stand-ins for device addresses
    d = (2, 3, 5, 7, 7, 4)
    for tr in ALL:
        assert q(*tr, *d, 0) > 0
    for tr in ((0, 32, 32), (64, 0, 32), (64, 32, 0), (32, 32, 32), (96, 32, 32), (128, 16, 64), (128, 128, 64), (128, 64, 128),
               (128, 64, 48), (256, 64, 64), (-64, 32, 32), (64, 33, 32)):
        assert q(*tr, *d, 0) == 0, tr
        assert f(a, a, a, a, *tr, *d, a, a, a, a, big, 0, None) == BAD_ARG
        assert b"c0" in L.v2ce_last_error()
    ok = (128, 64, 64)
    assert q(*ok, 0, 3, 5, 7, 7, 4, 0) == 0 and q(*ok, 2, 0, 5, 7, 7, 4, 0) == 0 and q(*ok, 2, 3, 0, 7, 7, 4, 0) == 0
    assert q(*ok, 2, 3, 5, 0, 7, 4, 0) == 0 and q(*ok, 2, 3, 5, 7, 6, 4, 0) == 0 and q(*ok, 2, 3, 5, 7, 7, 3, 0) == 0
    assert q(*ok, *d, -1) == 0
    assert q(*ok, 4096, 4096, 16, 16, 16, 8, 0) == 0                     # 2^32 positions
    assert q(*ok, 1, 1 << 20, 1, 1 << 10, 1 << 14, 1 << 9, 0) == 0       # B L H pitch = 2^34
    assert q(*ok, 1, 1 << 20, 1, 2, 2, 1 << 14, 0) == 0                  # B L H0 pitch0 = 2^34
    # refused before anything is launched (the addresses below are never dereferenced)
    assert f(a, a, a, a, *ok, 2, 3, 5, 7, 6, 4, a, a, a, a, big, 0, None) == BAD_ARG       # pitch < W
    assert f(a, a, a, a, *ok, 2, 3, 5, 7, 7, 3, a, a, a, a, big, 0, None) == BAD_ARG       # pitch0 < W0
    assert f(a, a, a, a, *ok, *d, a, a, a, a, big, -1, None) == BAD_ARG
    assert f(a, a, a, a, *ok, *d, None, None, None, a, big, 0, None) == BAD_ARG and b"no output" in L.v2ce_last_error()
    for args in ((None, a, a, a, a, a, a, a), (a, None, a, a, a, a, a, a), (a, a, None, a, a, a, a, a), (a, a, a, None, a, a, a, a),
                 (a, a, a, None, None, None, a, a), (a, a, a, a, a, a, a, None)):
        x0, x1, g1, gd, dw, ds, db, ws = args
        assert f(x0, x1, g1, gd, *ok, *d, dw, ds, db, ws, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error(), args
    for k in range(4):
        ptrs = [a] * 4
        ptrs[k] = a + 4
        assert f(*ptrs, *ok, *d, a, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()
    assert f(a, a, a, a, *ok, *d, a, a, a, a + 4, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # workspace
    need = q(*ok, *d, 0)
    assert f(a, a, a, a, *ok, *d, a, a, a, a, need - 4, 0, None) == WORKSPACE and b"workspace too small" in L.v2ce_last_error()


def test_integer_truths_of_check_a_are_integers_below_2_to_24():
    """With values 1 .. 3 a product is at most 9.  Below 2^24 every integer is an f32, so an fmaf chain, a sum of such chains
    in f64 and the one rounding of the store are exact in any order."""
    top = G.INT_MAX ** 2
    for shape in list(R.SMALL) + [R.WALK]:
        n = int(np.prod(shape))
        assert n * top < 2 ** 24 and n * G.INT_MAX < 2 ** 24              # d_weight, d_short; d_short_bias
    assert hip.UPWGRAD_CHAIN * top < 2 ** 24                             # one f32 chain
    for c0, c1, cout in R.TRIPLES:
        z = R.inputs((2, 3, 5, 7), c0, c1, cout, True, 303)
        for k, v in R.wgrad_truth(z["x0"], z["x1"], z["g1"], z["gd"]).items():
            assert torch.equal(v, v.round()) and 0 < float(v.max()) < 2 ** 24, k


def test_command_line_and_groups():
    p = finetune.build_parser()
    for choice in ("head", "tail", "tail_norms", "last_block", "dec2_conv2", "dec2_block"):
        assert p.parse_args(["--gt_events", "e.npz", "--train", choice]).train == choice
    with pytest.raises(SystemExit):
        p.parse_args(["--gt_events", "e.npz", "--train", "dec1_block"])
    assert finetune.DEC2_CONV_GROUPS == ("pred", "conv2", "bn2", "bn1", "bnd", "conv1", "convd", "dec2_conv2", "dec2_bn2")
    assert finetune.DEC2_BLOCK_GROUPS == finetune.DEC2_CONV_GROUPS + ("dec2_conv1", "dec2_convd", "dec2_bn1", "dec2_bnd")
    with pytest.raises(ValueError, match="train must be"):
        finetune.fit_dec2_block(None, None, None, train=("dec1_conv2",), steps=1, lr=1e-3)


def test_goldens_are_small_and_complete():
    files = sorted(glob.glob(os.path.join(B2.GOLD, "*.npz")))
    assert len(files) >= 8 and all(os.path.getsize(p) <= SIZE_CAP == 300_000 for p in files)
    assert sum(os.path.getsize(p) for p in files) <= 8 * 2 ** 20
    assert {os.path.basename(p).split(".")[0] for p in files} == set(B2.CASES) | {"consts"}
    for name, (B, L, H, W) in B2.CASES.items():
        z = B2.load_case(name)
        assert set(B2.PARAMS) | {"x0", "x1", "upstream", "ref64_out"} | {"ref64_" + k for k in B2.BLOCK_GRADS} <= set(z), name
        assert z["x0"].shape == (B, 128, L, (H + 1) // 2, (W + 1) // 2) and z["x1"].shape == (B, 64, L, H, W)
        assert z["upstream"].shape == z["ref64_out"].shape == (B, 64, L, H, W) and z["x0"].dtype == np.float32
        assert z["weight_bar1"].shape == (64, 192, 3, 3, 3) and z["ref64_out"].dtype == np.float64


@pytest.mark.parametrize("name", sorted(B2.CASES))
def test_restatement_gives_the_references_gradients(name):
    z = B2.load_case(name)
    p = {k: z[k] for k in B2.PARAMS}
    f = B2.block_forward(z["x0"], z["x1"], p)
    g = B2.block_grads(z["x0"], z["x1"], p, z["upstream"], f)
    for pre in (f["pre1"], f["pre"]):
        assert not (np.abs(pre) < B2.MARGIN).any() and 0.2 < (pre > 0).mean() < 0.8
    assert np.array_equal(f["out"] > 0, z["ref64_out"] > 0)
    assert np.abs(f["out"] - z["ref64_out"]).max() <= 1e-11 * np.abs(z["ref64_out"]).max()
    for k in B2.BLOCK_GRADS:
        want, have = z["ref64_" + k], g[k]
        if k in B2.SEAM_ONLY.get(name, ()):
            have = have[:, B2.SEAM]
        assert have.shape == want.shape and np.abs(want).max() > 0, k
        assert np.abs(have - want).max() <= 1e-11 * np.abs(want).max(), (name, k)
    for k, key in (("u1a", "ref64_u1_after"), ("v1a", "ref64_v1_after"), ("u2a", "ref64_u2_after"), ("v2a", "ref64_v2_after")):
        assert np.abs(f[k] - z[key]).max() <= 1e-13, k
