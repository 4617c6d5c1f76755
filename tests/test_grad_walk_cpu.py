"""CPU side of the full-grid walk tests of the five gradient kernels (tests/test_gpu_grad_walks.py): the torch f64 ports of
tests/grad_walk_ref.py against the numpy restatements that torch's f64 goldens validate, the walk table's properties from
the host-only size queries, the exactness margin of the integer data, and what a dropped or repeated tile does to the
truth.

Why integer data.  The weight-gradient contract is ulp32 + 4096 2^-24 S + N 2^-52 S, about 2.4e-4 of an element's sum of
|terms| S.  On standard-normal data at the deep row one tile of 128 positions adds a random sum of about +-11 to an element
whose bound is about 85: ``test_contract_bound_on_normal_data_cannot_see_a_lost_tile`` shows that the truth with a tile
zeroed, or counted twice, stays inside the contract bound of the full truth in every element, so a kernel that loses a tile
would pass check B.  On integers 1 .. 3 every term is a positive integer, every sum the kernels form is exact
(``test_integer_sums_are_exact_in_f32``), and a tile that is dropped, repeated or paired with the wrong tap moves every
output it feeds by at least 1 (``test_lost_or_repeated_tile_changes_every_output_it_feeds``): only bit-exact equality with
the f64 truth passes."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_walk_ref as G
from tests import last_block_dgrad_ref as BD
from tests import last_block_ref as BR
from tests import last_conv_dgrad_ref as CD
from tests import last_conv_ref as CR
from tests import pred_head_ref as PR
from v2ce_toolbox_amd import hip

SMALL = [(2, 3, 5, 7), (1, 2, 3, 70)]
OPS = ("conv32_wgrad", "conv32_dgrad", "convup_wgrad", "convup_dgrad", "pred_head_grads")
COUT = 20


def inputs(shape, exact, seed):
    return {**G.walk_inputs(shape, exact, seed), **G.head_inputs(shape, exact, seed + 1, COUT)}


def numpy_truth(op, z, use_y):
    n = {k: v.numpy() for k, v in z.items()}
    y = n["y"] if use_y else None
    if op == "conv32_wgrad":
        return CR.wgrad(n["x"], y, n["upstream"])
    if op == "conv32_dgrad":
        return CD.dgrad(n["weight"], y, n["upstream"])
    if op == "convup_wgrad":
        return BR.wgrad(n["x0"], n["x1"], n["g1"], n["gd"])
    if op == "convup_dgrad":
        return BD.dgrad(n["weight_up"], n["short"], n["g1"], n["gd"])
    yh = n["y_head"] if use_y else np.ones_like(n["y_head"])
    return PR.grads(n["feat"], yh, n["up_head"], n["w_head"])


def torch_truth(op, z, use_y=True):
    y = z["y"] if use_y else None
    if op == "conv32_wgrad":
        return G.conv32_wgrad(z["x"], y, z["upstream"])
    if op == "conv32_dgrad":
        return G.conv32_dgrad(z["weight"], y, z["upstream"])
    if op == "convup_wgrad":
        return G.convup_wgrad(z["x0"], z["x1"], z["g1"], z["gd"])
    if op == "convup_dgrad":
        return G.convup_dgrad(z["weight_up"], z["short"], z["g1"], z["gd"])
    return G.pred_head_grads(z["feat"], z["y_head"] if use_y else None, z["up_head"], z["w_head"])


# kernel -> {summed output: its sum of |terms|}
PAIRS = {
    "conv32_wgrad": {"d_weight": "abs_weight", "d_shift": "abs_shift"},
    "conv32_dgrad": {"d_x": "abs_x"},
    "convup_wgrad": {"d_weight": "abs_weight", "d_short": "abs_short", "d_short_bias": "abs_short_bias"},
    "convup_dgrad": {"d_x0": "abs_x0", "d_x1": "abs_x1"},
    "pred_head_grads": {"d_weight": "abs_weight", "d_bias": "abs_bias"},
}


@pytest.mark.parametrize("exact", [True, False], ids=["integers", "normals"])
@pytest.mark.parametrize("use_y", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", OPS)
def test_port_matches_the_numpy_restatement(op, shape, use_y, exact):
    """Both sum the same terms in f64, in two orders: an element's two values are each within n 2^-53 S of the exact sum of
    its n terms (S = their absolute sum), so they differ by at most n 2^-52 S.  n <= the number of positions for the
    weight gradients and 4 * 896 for the input gradients; the larger of the two serves every output."""
    z = inputs(shape, exact, 11)
    want, got = numpy_truth(op, z, use_y), torch_truth(op, z, use_y)
    n = max(int(np.prod(shape)), 4 * hip.UPDGRAD_TERMS)
    assert set(got) == set(want), op
    for out, terms in PAIRS[op].items():
        tol = n * 2.0 ** -52 * want[terms]
        for k in (out, terms):
            g = got[k].numpy()
            assert g.dtype == np.float64 and g.shape == want[k].shape, (op, k)
            assert np.all(np.abs(g - want[k]) <= tol), (op, k, float(np.abs(g - want[k]).max()))
        assert want[terms].min() >= 0 and want[terms].max() > 0
    if op == "conv32_dgrad":
        assert np.array_equal(got["d_res"].numpy(), want["d_res"])
        if use_y:
            assert (want["d_res"] == 0).mean() > 0.3                  # the mask is in force
    if op == "convup_dgrad":
        assert np.array_equal(got["n_x0"].numpy(), want["n_x0"])
        assert np.all(np.abs(got["d_X"].numpy() - want["d_X"]) <= n * 2.0 ** -52 * np.abs(want["d_X"]).max())
    if op == "pred_head_grads":
        assert np.all(np.abs(got["d_feat"].numpy() - want["d_feat"]) <= COUT * 2.0 ** -52 * np.abs(want["d_feat"]).max())
    if exact:                                                         # integers: both are the exact sums
        for out in PAIRS[op]:
            assert np.array_equal(got[out].numpy(), want[out]), (op, out)


def test_signed_zeros_of_y_close_the_mask():
    z = G.walk_inputs(SMALL[1], True, seed=5)
    y = z["y"].numpy()
    pos, neg = (y == 0) & ~np.signbit(y), (y == 0) & np.signbit(y)
    assert 0.002 < pos.mean() < 0.03 and 0.002 < neg.mean() < 0.03
    m = G.masked(z["y"], z["upstream"]).numpy()
    assert not m[pos].any() and not m[neg].any() and np.array_equal(m > 0, y > 0)
    assert set(np.unique(z["upstream"].numpy())) == {1.0, 2.0, 3.0}


# ---------------------------------------------------------------------------------------------------------------------
# the walk table

def queries():
    L = hip.lib()
    return (L.v2ce_conv32_wgrad_workspace_bytes, L.v2ce_conv32_dgrad_workspace_bytes, L.v2ce_convup_wgrad_workspace_bytes,
            L.v2ce_convup_dgrad_workspace_bytes, L.v2ce_pred_head_grads_workspace_bytes)


@pytest.mark.parametrize("row", sorted(G.WALKS))
def test_walk_table_rows_put_the_default_grid_at_its_cap_on_uneven_shares(row):
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d, _nearest_is_half
    B, Lq, H, W = shape = G.WALKS[row]
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    pitch, pitch0 = G.pitch_of(W), G.pitch_of(W0)
    assert (pitch, pitch0) == (V2ce3d._pitch(W), V2ce3d._pitch(W0)) and pitch > W    # the activation pitch; padding columns exist
    assert _nearest_is_half(H0, H) and _nearest_is_half(W0, W)
    q_w, q_d, q_uw, q_ud, q_h = queries()
    tiles = G.conv_tiles(*shape)
    assert tiles == {"wide": 1710, "deep": 8496}[row]
    # the grid-sized workspaces: the default is the cap's, and one workgroup (one share) fewer is smaller
    assert q_w(*shape, pitch, 0) == q_w(*shape, pitch, G.CAP_CONV32) > q_w(*shape, pitch, G.CAP_CONV32 - 1) > 0
    assert q_w(*shape, pitch, 0) >= G.CAP_CONV32 * (27 * 32 * 32 + 32) * 8
    cap = 3 * G.CAP_UPWGRAD_SHARES
    assert q_uw(*shape, pitch, pitch0, 0) == q_uw(*shape, pitch, pitch0, cap) > q_uw(*shape, pitch, pitch0, cap - 1) > 0
    assert q_uw(*shape, pitch, pitch0, cap + 3) == q_uw(*shape, pitch, pitch0, 0)
    # the input gradients' workspaces hold the repacked weights only: the grid is the documented min(tiles, 256)
    assert q_d(*shape, pitch, 0) == q_d(*shape, pitch, 1) == q_d(1, 1, 1, 1, 1, 0) > 0
    assert q_ud(*shape, pitch, pitch0, 0) == q_ud(*shape, pitch, pitch0, 1) == q_ud(1, 1, 1, 1, 1, 1, 0) > 0
    assert tiles > G.CAP_CONV32 and tiles > G.CAP_UPDGRAD
    grids = {"conv32_wgrad": G.CAP_CONV32, "conv32_dgrad": G.CAP_CONV32, "convup_wgrad": G.CAP_UPWGRAD_SHARES,
             "convup_dgrad": G.CAP_UPDGRAD // 3, f"all at max_workgroups={G.OTHER_GRID}": G.OTHER_GRID,
             f"convup at max_workgroups={G.OTHER_GRID}": G.OTHER_GRID // 3}
    for name, shares in grids.items():
        sizes = G.share_sizes(tiles, shares)
        assert sum(sizes) == tiles and min(sizes) >= 2 and tiles % shares != 0 and max(sizes) == min(sizes) + 1, name
    frame, tile_row = ((H + 1) // 2) * ((W + 63) // 64), (W + 63) // 64
    for shares in (G.CAP_CONV32, G.CAP_UPWGRAD_SHARES, G.OTHER_GRID):
        starts = [b * tiles // shares for b in range(1, shares)]
        assert any(s % frame for s in starts) and any(s % (frame * Lq) for s in starts)    # mid-frame, mid-sequence
        if tile_row > 1:
            assert any(s % tile_row for s in starts)                                         # mid-row of tiles
    assert H % 2 == 1                                                 # the last tile row holds one row
    if row == "wide":
        assert W % 64 == 3 and (H0, W0) == (38, 66)                   # the last tile column holds three columns
        n = G.head_tiles(*shape)
        assert n == 1152 and B * Lq * H * W % G.HEAD_TILE != 0
        for cout in G.HEAD_COUTS:
            # the head's query takes no grid: a shape of exactly 512 (511) tiles stands for the cap (one workgroup fewer)
            at_cap, below = (q_h(1, 1, cout, rows, G.HEAD_TILE, G.HEAD_TILE) for rows in (G.CAP_HEAD, G.CAP_HEAD - 1))
            assert q_h(B, Lq, cout, H, W, pitch) == at_cap > below > 0 and at_cap == q_h(4, 16, cout, 260, 346, 352)
        sizes = G.share_sizes(n, G.CAP_HEAD)
        assert min(sizes) == 2 and max(sizes) == 3
        assert sorted(set(G.share_sizes(tiles, G.CAP_CONV32))) == [6, 7] and sorted(set(G.share_sizes(tiles, 85))) == [20, 21]
    else:
        assert (H0, W0) == (177, 33)
        for chain, shares, want in ((hip.WGRAD_CHAIN, G.CAP_CONV32, [33, 34]),
                                    (hip.UPWGRAD_CHAIN, G.CAP_UPWGRAD_SHARES, [99, 100])):
            per, sizes = chain // 128, G.share_sizes(tiles, shares)
            assert sorted(set(sizes)) == want
            assert min(sizes) > per and max(sizes) % per != 0 and min(sizes) % per != 0    # flushes, then a partial chain


def test_integer_sums_are_exact_in_f32():
    """With |values| <= 3 a product is at most 9.  Below 2^24 every integer is an f32, so an fmaf chain, a sum of such
    chains in f64 and the one rounding of the store are exact, in any order; the same holds for the plain f32 additions of
    the input gradients."""
    top = G.INT_MAX ** 2
    for shape in G.WALKS.values():
        n = int(np.prod(shape))
        assert n * top < 2 ** 24                                      # every final sum: d_weight, d_short, the head's d_weight
        assert n * G.INT_MAX < 2 ** 24                                # d_shift, d_short_bias, d_bias
    assert max(hip.WGRAD_CHAIN, hip.UPWGRAD_CHAIN) * top < 2 ** 24   # one f32 chain
    assert hip.DGRAD_TERMS * top < 2 ** 24                           # d_x
    assert 4 * hip.UPDGRAD_TERMS * top < 2 ** 24                     # d_x1, and d_x0 pooled over up to four positions
    assert max(G.HEAD_COUTS) * top < 2 ** 24                         # the head's d_feat


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: a tile dropped or counted twice

SENS = (2, 2, 3, 67)                       # 16 tiles; the last tile row holds one row, the last tile column three columns
CARRIERS = {"conv32_wgrad": ("upstream",), "conv32_dgrad": ("upstream",), "convup_wgrad": ("g1", "gd"),
            "convup_dgrad": ("g1", "gd"), "pred_head_grads": ("up_head",)}


def tile_mask(op, index):
    """[B, 1, L, H, W] bool: the positions of tile `index` of `op`'s walk."""
    B, L, H, W = SENS
    m = torch.zeros((B, 1, L, H, W), dtype=torch.bool)
    if op == "pred_head_grads":
        flat = m.permute(1, 0, 2, 3, 4).reshape(-1)
        flat[index * G.HEAD_TILE:(index + 1) * G.HEAD_TILE] = True
        return flat.reshape(1, B, L, H, W).permute(1, 0, 2, 3, 4)
    b, l, h0, h1, w0, w1 = G.tile_of(SENS, index)
    m[b, 0, l, h0:h1, w0:w1] = True
    return m


@functools.lru_cache(maxsize=None)
def sens_inputs(exact):
    return inputs(SENS, exact, 23)


def with_tile(op, z, index, factor, only=False):
    """The inputs with the gradient-carrying tensors scaled by `factor` at the tile (only: and zeroed everywhere else)."""
    m, z2 = tile_mask(op, index), dict(z)
    for k in CARRIERS[op]:
        z2[k] = torch.where(m, z[k] * factor, torch.zeros_like(z[k]) if only else z[k])
    return z2


def n_tiles(op):
    return G.head_tiles(*SENS) if op == "pred_head_grads" else G.conv_tiles(*SENS)


@pytest.mark.parametrize("op", OPS)
def test_lost_or_repeated_tile_changes_every_output_it_feeds(op):
    z, last = sens_inputs(True), n_tiles(op) - 1
    full = torch_truth(op, z, use_y=False)
    outs = list(PAIRS[op]) + (["d_res"] if op == "conv32_dgrad" else []) + (["d_feat"] if op == "pred_head_grads" else [])
    if op != "pred_head_grads":
        b, l, h0, h1, w0, w1 = G.tile_of(SENS, last)
        assert (h1 - h0, w1 - w0) == (1, 3) and G.conv_tiles(*SENS) == 16         # the ragged last tile
    else:
        assert int(np.prod(SENS)) % G.HEAD_TILE != 0
    for index in (0, last // 2, last):
        alone = torch_truth(op, with_tile(op, z, index, 1.0, only=True), use_y=False)
        for factor in (0.0, 2.0):                                    # dropped; counted twice
            other = torch_truth(op, with_tile(op, z, index, factor), use_y=False)
            for k in outs:
                fed = alone[k] != 0
                assert fed.any() and torch.equal(other[k] - full[k], (factor - 1.0) * alone[k]), (op, k, index)   # linear, exact
                # every output the tile feeds moves by at least 1, and stays an f32: bit-exact equality cannot hold
                assert torch.equal(other[k].float() != full[k].float(), fed), (op, k, index)
                assert torch.equal(other[k].float().double(), other[k]) and (alone[k][fed] >= 1).all()
        check_fed_region(op, index, alone)


def check_fed_region(op, index, alone):
    """What a tile feeds, from the geometry alone: all positive data, so a reachable output is a non-zero one."""
    B, L, H, W = SENS
    if op == "pred_head_grads":
        n = min(G.HEAD_TILE, B * L * H * W - index * G.HEAD_TILE)
        assert (alone["d_weight"] != 0).all() and (alone["d_bias"] != 0).all()
        assert int((alone["d_feat"] != 0).sum()) == 32 * n
        return
    b, l, h0, h1, w0, w1 = G.tile_of(SENS, index)
    if op.endswith("wgrad"):
        # tap (kt, kh, kw) is fed when some position of the tile has its shifted partner inside the tensor
        ok = lambda lo, hi, k, size: any(0 <= p + k - 1 < size for p in range(lo, hi))
        taps = torch.tensor([[[ok(l, l + 1, kt, L) and ok(h0, h1, kh, H) and ok(w0, w1, kw, W) for kw in range(3)]
                              for kh in range(3)] for kt in range(3)])
        assert torch.equal((alone["d_weight"] != 0), taps.expand_as(alone["d_weight"]))
        for k in ("d_shift", "d_short", "d_short_bias"):
            assert k not in alone or (alone[k] != 0).all()
        return
    # input gradients: the tile dilated by one position, clipped to the tensor, in every channel
    box = lambda lo, hi, size: (max(lo - 1, 0), min(hi + 1, size))
    (la, lb), (ha, hb), (wa, wb) = box(l, l + 1, L), box(h0, h1, H), box(w0, w1, W)
    want = torch.zeros((B, 1, L, H, W), dtype=torch.bool)
    want[b, 0, la:lb, ha:hb, wa:wb] = True
    if op == "conv32_dgrad":
        assert torch.equal(alone["d_x"] != 0, want.expand_as(alone["d_x"]))
        assert torch.equal(alone["d_res"] != 0, tile_mask(op, index).expand_as(alone["d_res"]))
    else:
        assert torch.equal(alone["d_x1"] != 0, want.expand_as(alone["d_x1"]))
        src = G.pooled(want.double()) != 0
        assert torch.equal(alone["d_x0"] != 0, src.expand_as(alone["d_x0"]))


def test_contract_bound_on_normal_data_cannot_see_a_lost_tile():
    """The deep row's shortcut weight gradient (one tap: the cheapest of the chained sums, statistically like any tap of
    d_weight) on standard normals: the truth with a first, a middle or the ragged last tile zeroed or counted twice is
    inside the contract bound around the full truth in EVERY element.  Reasoning, not a measurement of the kernel: S is
    about N E|g| E|X| = 550 680 * 0.64 = 3.5e5, the bound 2.44e-4 S = 85; a tile adds a sum of 128 products of unit
    variance, +-11, and the largest of 3072 such sums is about 4 sigma = 45.  Check B alone would pass such a kernel."""
    shape = G.WALKS["deep"]
    B, L, H, W = shape
    gen = torch.Generator().manual_seed(31)
    x0, x1 = G.normals(gen, (B, 64, L, (H + 1) // 2, (W + 1) // 2)), G.normals(gen, (B, 32, L, H, W))
    gd = G.normals(gen, (B, 32, L, H, W))
    full = G.convup_wgrad(x0, x1, None, gd)
    n = B * L * H * W
    bound = BR.wgrad_bound(full["d_short"].numpy(), full["abs_short"].numpy(), n, hip.UPWGRAD_CHAIN)
    tiles = G.conv_tiles(*shape)
    worst = 0.0
    for index in (0, tiles // 2, tiles - 1):
        b, l, h0, h1, w0, w1 = G.tile_of(shape, index)
        for factor in (0.0, 2.0):
            g2 = gd.clone()
            g2[b, :, l, h0:h1, w0:w1] *= factor
            diff = np.abs(G.convup_wgrad(x0, x1, None, g2)["d_short"].numpy() - full["d_short"].numpy())
            assert diff.max() > 0
            worst = max(worst, float((diff / bound).max()))
            assert np.all(diff <= bound), (index, factor, float((diff / bound).max()))
    print(f"a lost or repeated tile moves d_short by at most {worst:.3f} of the contract bound")
    assert worst < 1.0
