"""CPU side of the tests of v2ce_convn_wgrad / v2ce_convn_dgrad (include/v2ce_hip_convngrad.h, tests/test_gpu_convngrad.py):
the truths of tests/convn_ref.py against torch.nn.grad in f64, the header's symbols, the refusals and the share arithmetic
from the host-only size queries, the exactness margin of the integer data of check A, and what a lost tile or a swapped
channel group does to the truth."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import convn_ref as R
from tests import grad_walk_ref as G
from v2ce_toolbox_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "v2ce_hip_convngrad.h"
BAD_ARG, WORKSPACE = -1, -4
ALL = R.PAIRS + ((32, 32),)
PARTIAL = (27 * 32 * 32 + 32) * 8                                    # f64 bytes of one workgroup's partial sums


@pytest.mark.parametrize("use_y", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 3, 6)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin,cout", ALL)
def test_truths_match_numpy_and_torch_nn_grad(cin, cout, shape, use_y):
    """Three statements of the same f64 sums: the device truth of the GPU tests (one matmul per tap), the numpy restatement
    of the header's formulas (term by term), and torch.nn.grad on the masked upstream.  Each is within n 2^-53 S of the exact
    sum of an element's n terms, so two of them differ by at most n 2^-52 S."""
    z = R.inputs(shape, cin, cout, False, 17)
    y = z["y"] if use_y else None
    m = G.masked(y, z["upstream"])
    tw, td = R.wgrad_truth(z["x"], y, z["upstream"]), R.dgrad_truth(z["weight"], y, z["upstream"])
    nw = R.wgrad_np(z["x"].numpy(), None if y is None else y.numpy(), z["upstream"].numpy())
    nd = R.dgrad_np(z["weight"].numpy(), None if y is None else y.numpy(), z["upstream"].numpy())
    x64, w64 = z["x"].double(), z["weight"].double()
    ref_w = torch.nn.grad.conv3d_weight(x64, w64.shape, m, padding=1)
    ref_x = torch.nn.grad.conv3d_input(x64.shape, w64, m, padding=1)
    n = max(int(np.prod(shape)), 27 * cout)
    tol_w, tol_x = n * 2.0 ** -52 * tw["abs_weight"].numpy(), n * 2.0 ** -52 * td["abs_x"].numpy()
    assert tuple(tw["d_weight"].shape) == (cout, cin, 3, 3, 3) and tuple(td["d_x"].shape) == tuple(z["x"].shape)
    for other in (nw["d_weight"], ref_w.numpy()):
        assert np.all(np.abs(tw["d_weight"].numpy() - other) <= tol_w)
    for other in (nd["d_x"], ref_x.numpy()):
        assert np.all(np.abs(td["d_x"].numpy() - other) <= tol_x)
    assert np.all(np.abs(tw["d_shift"].numpy() - nw["d_shift"]) <= n * 2.0 ** -52 * tw["abs_shift"].numpy())
    assert np.all(np.abs(tw["d_shift"].numpy() - m.sum(dim=(0, 2, 3, 4)).numpy()) <= n * 2.0 ** -52 * tw["abs_shift"].numpy())
    assert np.array_equal(td["d_res"].numpy(), nd["d_res"]) and np.array_equal(nd["d_res"], m.numpy())
    assert tw["abs_weight"].min() >= 0 and tw["abs_weight"].max() > 0 and td["abs_x"].max() > 0
    if use_y:
        assert (nd["d_res"] == 0).mean() > 0.3                         # the mask is in force


def declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_symbols_of_the_convngrad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.CONVNGRAD_EXPORTS) and len(set(hip.CONVNGRAD_EXPORTS)) == len(hip.CONVNGRAD_EXPORTS)
    older = (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS, hip.CONVUPGRAD_EXPORTS,
             hip.CONVUPDGRAD_EXPORTS)
    for other in older:
        assert not set(hip.CONVNGRAD_EXPORTS) & set(other)
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != HEADER]
    assert len(others) >= 7
    for other in others:
        assert not any(s in open(other).read() for s in syms), other
    # the header names the older entries by file only (their own tests look for their symbols in every other header)
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    assert not any(s in own for s in hip.CONVGRAD_EXPORTS + hip.CONVDGRAD_EXPORTS + hip.CONVUPGRAD_EXPORTS + hip.CONVUPDGRAD_EXPORTS)
    make = open(os.path.join(ROOT, "v2ce-toolbox_amd", "csrc", "Makefile")).read()
    links = [ln for ln in make.splitlines() if "-shared" in ln]
    assert len(links) >= 6 and all("convnwgrad.o" in ln and "convndgrad.o" in ln or "$(OBJS)" in ln for ln in links)
    assert "convnwgrad.o convndgrad.o" in [ln for ln in make.splitlines() if ln.startswith("OBJS")][0]


def test_size_queries_follow_the_documented_shares():
    L = hip.lib()
    qw, qd = L.v2ce_convn_wgrad_workspace_bytes, L.v2ce_convn_dgrad_workspace_bytes
    q32w, q32d = L.v2ce_conv32_wgrad_workspace_bytes, L.v2ce_conv32_dgrad_workspace_bytes
    up256 = lambda n: (n + 255) // 256 * 256
    shapes = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 7), (1, 3, 20, 70, 96), (1, 16, 130, 173, 192), R.WALK + (G.pitch_of(R.WALK[3]),)]
    for cin, cout in ALL:
        p = R.pairs_of(cin, cout)
        for d in shapes:
            tiles = G.conv_tiles(*d[:4])
            for cap in (0, 1, 2, 3, 4, 5, 8, 97, 255, 256, 1000):
                assert qw(cin, cout, *d, cap) == up256(R.wgrad_shares(cin, cout, tiles, cap) * p * PARTIAL), (cin, cout, d, cap)
                assert qd(cin, cout, *d, cap) == up256(27 * cin * cout * 4)                      # the grid needs nothing
            if (cin, cout) == (32, 32):
                assert all(qw(32, 32, *d, cap) == q32w(*d, cap) and qd(32, 32, *d, cap) == q32d(*d, cap) for cap in (0, 3, 97, 300))
    # dec2's shape: the default grid is 256 workgroups whatever the pairs are
    d = (1, 16, 130, 173, 192)
    assert {qw(cin, cout, *d, 0) for cin, cout in ALL} == {up256(256 * PARTIAL)}


def test_walk_shape_puts_the_default_grids_at_their_caps_on_uneven_shares():
    B, Lq, H, W = R.WALK
    L = hip.lib()
    qw = L.v2ce_convn_wgrad_workspace_bytes
    pitch = G.pitch_of(W)
    tiles = G.conv_tiles(*R.WALK)
    assert tiles == 396 and pitch > W and H % 2 == 1 and W % 64 == 3      # a one-row last tile row, a three-column last tile
    frame, tile_row = ((H + 1) // 2) * ((W + 63) // 64), (W + 63) // 64
    for cin, cout in R.PAIRS:
        p, g = R.pairs_of(cin, cout), cin // R.GROUP
        cap_w, cap_d = R.CAP // p, R.CAP // g
        assert tiles > cap_w and tiles > cap_d
        assert R.wgrad_shares(cin, cout, tiles) == cap_w and R.dgrad_shares(cin, tiles) == cap_d
        # the workspace is the cap's, and one share fewer is smaller
        assert qw(cin, cout, *R.WALK, pitch, 0) == qw(cin, cout, *R.WALK, pitch, R.CAP) == qw(cin, cout, *R.WALK, pitch, 10 ** 6)
        assert qw(cin, cout, *R.WALK, pitch, 0) > qw(cin, cout, *R.WALK, pitch, R.CAP - p) > 0
        for shares in (cap_w, cap_d, R.wgrad_shares(cin, cout, tiles, R.PRIME_GRID), R.dgrad_shares(cin, tiles, R.PRIME_GRID)):
            sizes = G.share_sizes(tiles, shares)
            assert sum(sizes) == tiles and tiles % shares != 0 and max(sizes) == min(sizes) + 1 and min(sizes) >= 1, (cin, cout, shares)
            starts = [b * tiles // shares for b in range(1, shares)]
            assert any(s % frame for s in starts) and any(s % (frame * Lq) for s in starts) and any(s % tile_row for s in starts)
    # the one-share row of the small shapes: 60 tiles, a full chain of 32 tiles and a partial one of 28
    shape = (1, 3, 20, 70)
    assert R.SMALL[shape] == 1 and G.conv_tiles(*shape) == 60 and hip.WGRAD_CHAIN // 128 == 32
    for cin, cout in R.PAIRS:
        assert R.wgrad_shares(cin, cout, 60, R.pairs_of(cin, cout)) == 1
        assert qw(cin, cout, *shape, 96, R.pairs_of(cin, cout)) == R.pairs_of(cin, cout) * PARTIAL


def test_refusals_without_gpu():
    L = hip.lib()
    a, big = 4096, 1 << 30                                              # aligned stand-ins for device addresses
    d = (2, 3, 5, 7, 7)
    for q, f, first in ((L.v2ce_convn_wgrad_workspace_bytes, L.v2ce_convn_wgrad, "x"),
                        (L.v2ce_convn_dgrad_workspace_bytes, L.v2ce_convn_dgrad, "weight")):
        for cin, cout in ALL:
            assert q(cin, cout, *d, 0) > 0
        for cin, cout in ((0, 32), (32, 0), (16, 32), (48, 64), (64, 96), (128, 64), (-32, 32), (33, 32)):
            assert q(cin, cout, *d, 0) == 0, (cin, cout)
            assert f(a, a, a, cin, cout, *d, a, a, a, big, 0, None) == BAD_ARG
            assert b"cin" in L.v2ce_last_error()
        ok = (64, 64)
        assert q(*ok, 0, 3, 5, 7, 7, 0) == 0 and q(*ok, 2, 0, 5, 7, 7, 0) == 0 and q(*ok, 2, 3, 0, 7, 7, 0) == 0
        assert q(*ok, 2, 3, 5, 0, 7, 0) == 0 and q(*ok, 2, 3, 5, 7, 6, 0) == 0 and q(*ok, *d, -1) == 0
        assert q(*ok, 4096, 4096, 16, 16, 16, 0) == 0                    # 2^32 positions
        assert q(*ok, 1, 1 << 20, 1, 1 << 10, 1 << 14, 0) == 0           # B L H pitch = 2^34
        # refused before anything is launched (the addresses below are never dereferenced)
        assert f(a, a, a, *ok, 2, 3, 5, 7, 6, a, a, a, big, 0, None) == BAD_ARG       # pitch < W
        assert f(a, a, a, *ok, *d, a, a, a, big, -1, None) == BAD_ARG
        assert f(None, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, None, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, a, *ok, *d, a, a, None, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, a, *ok, *d, None, None, a, big, 0, None) == BAD_ARG and b"no output" in L.v2ce_last_error()
        assert f(a, a + 4, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # y
        assert f(a, a, a + 8, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # upstream
        assert f(a, a, a, *ok, *d, a, a, a + 4, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # workspace
        if first == "x":
            assert f(a + 4, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()
        else:
            assert f(a + 2, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # weight
            assert f(a, a, a, *ok, *d, a + 4, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # d_x
            assert f(a, a, a, *ok, *d, a, a + 8, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # d_res
        need = q(*ok, *d, 0)
        rc = f(a, a, a, *ok, *d, a, a, a, need - 4, 0, None)
        assert rc == WORKSPACE and b"workspace too small" in L.v2ce_last_error()


def test_integer_sums_of_check_a_are_exact_in_f32():
    """With values 1 .. 3 a product is at most 9.  Below 2^24 every integer is an f32, so an fmaf chain, a sum of such
    chains in f64, the one rounding of the store and the plain f32 additions of the input gradient are exact in any order."""
    top = G.INT_MAX ** 2
    for shape in list(R.SMALL) + [R.WALK]:
        n = int(np.prod(shape))
        assert n * top < 2 ** 24 and n * G.INT_MAX < 2 ** 24              # d_weight; d_shift
    assert hip.WGRAD_CHAIN * top < 2 ** 24                               # one f32 chain
    assert 27 * max(hip.CONVN_CHANNELS) * top < 2 ** 24                  # d_x


SENS = (2, 2, 3, 67)                       # 16 tiles; the last tile row holds one row, the last tile column three columns


def sens_truth(z):
    t = dict(R.wgrad_truth(z["x"], None, z["upstream"]))
    t.update(R.dgrad_truth(z["weight"], None, z["upstream"]))
    return {k: t[k] for k in ("d_weight", "d_shift", "d_x", "d_res")}


@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_lost_or_repeated_tile_moves_every_output_it_feeds(cin, cout):
    z = R.inputs(SENS, cin, cout, True, 23)
    full, last = sens_truth(z), G.conv_tiles(*SENS) - 1
    assert last == 15 and G.tile_of(SENS, last)[3] - G.tile_of(SENS, last)[2] == 1
    for index in (0, last // 2, last):
        b, l, h0, h1, w0, w1 = G.tile_of(SENS, index)
        m = torch.zeros((SENS[0], 1) + SENS[1:], dtype=torch.bool)
        m[b, 0, l, h0:h1, w0:w1] = True
        alone = sens_truth({**z, "upstream": torch.where(m, z["upstream"], torch.zeros_like(z["upstream"]))})
        for factor in (0.0, 2.0):                                       # zeroed; doubled
            other = sens_truth({**z, "upstream": torch.where(m, z["upstream"] * factor, z["upstream"])})
            for k in full:
                fed = alone[k] != 0
                assert fed.any() and torch.equal(other[k] - full[k], (factor - 1.0) * alone[k]), (k, index)
                assert torch.equal(other[k].float() != full[k].float(), fed), (k, index)
                assert torch.equal(other[k].float().double(), other[k]) and (alone[k][fed] >= 1).all()


def swap_groups(t, dim):
    """Channels 0 .. 31 and 32 .. 63 of dimension `dim` exchanged."""
    a, b = t.narrow(dim, 0, 32), t.narrow(dim, 32, 32)
    return torch.cat([b, a], dim=dim)


def ordered(t, dim):
    """Integers 1 .. 2 in channels 0 .. 31 of `dim` and the same plus one in channels 32 .. 63 (32 channels: as they are)."""
    if t.shape[dim] == 32:
        return t
    low = t.narrow(dim, 0, 32).clamp(max=2.0)
    return torch.cat([low, low + 1.0], dim=dim)


@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_swapped_channel_groups_move_every_output_they_feed(cin, cout):
    """A kernel that reads co group 1 where it should read co group 0 (or the ci groups alike) computes the truth of the
    swapped inputs.  Integer data whose second group is the first plus one (still 1 .. 3; check A's random integers make
    the groups differ in nearly every sum, this makes it every one): each output the exchanged group feeds differs from
    the truth by at least 1, so bit-exact equality cannot hold."""
    z = R.inputs((2, 3, 5, 7), cin, cout, True, 29)
    z = {"x": ordered(z["x"], 1), "upstream": ordered(z["upstream"], 1),
         "weight": 1.0 + (torch.arange(cout) >= 32).float().view(-1, 1, 1, 1, 1) + (torch.arange(cin) >= 32).float().view(1, -1, 1, 1, 1)
         + torch.zeros((cout, cin, 3, 3, 3))}
    assert all(set(np.unique(v.numpy())) <= {1.0, 2.0, 3.0} for v in z.values())
    full = sens_truth(z)
    moved = lambda a, b: bool(((a - b).abs() >= 1).all())
    if cout == 64:
        other = sens_truth({**z, "upstream": swap_groups(z["upstream"], 1)})              # m's co groups
        for k, dim in (("d_weight", 0), ("d_shift", 0), ("d_res", 1)):
            assert torch.equal(other[k], swap_groups(full[k], dim)) and moved(other[k], full[k]), k
        assert moved(other["d_x"], full["d_x"])                                          # against the weight's own order
        assert moved(sens_truth({**z, "weight": swap_groups(z["weight"], 0)})["d_x"], full["d_x"])
    if cin == 64:
        other = sens_truth({**z, "x": swap_groups(z["x"], 1)})                            # x's ci groups
        assert torch.equal(other["d_weight"], swap_groups(full["d_weight"], 1)) and moved(other["d_weight"], full["d_weight"])
        other = sens_truth({**z, "weight": swap_groups(z["weight"], 1)})                  # the weight's ci groups
        assert torch.equal(other["d_x"], swap_groups(full["d_x"], 1)) and moved(other["d_x"], full["d_x"])
