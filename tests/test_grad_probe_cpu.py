"""CPU side of the probe tests of the eleven gradient kernels (tests/test_gpu_grad_probes.py): the conditions on the data of
probes 1 and 3 that make their bit-exact assertions valid and sharp, the share arithmetic of probe 2 against the headers'
host-side restatements, and a numpy model of hypothetical weight-gradient kernels (tests/grad_probe_ref.py: model_element)
showing that the contract's kernel passes every assertion of probe 2 and that each faulty variant fails a named one.

The appended cases (v2ce_convc_wgrad and v2ce_convc_dgrad at (128, 128), (512, 32), (32, 512), (512, 512), v2ce_convupn_dgrad
at convupn_ref.TRIPLES) go through the same tests, and through those of their own slot tables, product widths and grids
(16 and 256 pairs) below.  Their conditions are proved by convolving in f64 like the others', not by counting terms.

The model describes kernels that do not exist; the GPU test never uses it as an expectation."""
import functools

import numpy as np
import pytest
import torch

from tests import convn_ref as R
from tests import convupn_ref as RU
from tests import grad_probe_ref as P
from tests import grad_walk_ref as G
from v2ce_toolbox_amd import hip

IDS = [P.case_id(c) for c in P.CASES]


# ---------------------------------------------------------------------------------------------------------------------
# probe 1

@functools.lru_cache(maxsize=None)
def p1(case):
    z = P.p1_inputs(case)
    return z, P.truth(case[0], z, case[1])


def changed_everywhere(case, z2, names, label, all_but=0.0):
    """Every non-zero element of the named outputs (all but the fraction `all_but`) differs between the truth and the truth of
    the altered inputs z2."""
    t, t2 = p1(case)[1], P.truth(case[0], z2, case[1])
    for name in names:
        live = t[name] != 0
        assert live.any(), (case, name)
        same = int((live & (t2[name] == t[name])).sum())
        assert same <= all_but * int(live.sum()), (case, label, name, f"{same} of {int(live.sum())} non-zero elements unchanged")


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_wide_integer_sums_are_exact_in_any_f32_order(case):
    """An element's sum of |terms| is below 2^24 and the truth is an f32; every output has non-zero elements and every
    channel of the upstream gradient is fed."""
    kind = case[0]
    z, t = p1(case)
    a = P.abs_truth(kind, z, case[1])
    for name in P.OUTPUTS[kind]:
        assert float(a[name].max()) < 2 ** 24, (case, name, float(a[name].max()))
        assert torch.equal(t[name].to(torch.float32).to(torch.float64), t[name]), (case, name)
        assert (t[name] != 0).any(), (case, name)
    for name in P.ROLES[kind]["up"]:
        assert (G.rows(z[name]) != 0).any(dim=1).all(), (case, name, "an output channel without a term")
    if kind in ("wgrad", "upwgrad"):                                   # two terms each: they meet in f64 or in one f32 chain
        for name in P.ROLES[kind]["up"]:
            assert ((G.rows(z[name]) != 0).sum(dim=1) == 2).all(), (case, name)


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_wide_integer_products_need_f32_precision(case):
    """Every product is an odd integer of at least 21 significant bits (all of the non-zero outputs hold one, more than the
    half asked for): the operands are odd, and the smallest |up| times the smallest |other| is at least 2^20."""
    kind = case[0]
    z = p1(case)[0]
    nz = lambda v: v[v != 0].abs()
    for name in P.ROLES[kind]["up"] + P.ROLES[kind]["other"]:
        assert (nz(z[name]) % 2 == 1).all(), (case, name)
    low_up = min(float(nz(z[n]).min()) for n in P.ROLES[kind]["up"])
    low_other = min(float(nz(z[n]).min()) for n in P.ROLES[kind]["other"])
    assert low_up * low_other >= 2 ** 20, (case, low_up, low_other)
    assert low_up >= 2 ** 11 and low_other >= (2 ** 10 if kind == "updgrad" else 2 ** 11)   # 12 bits; 11: the pooled weights


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_a_precision_downgrade_changes_every_nonzero_output(case):
    """The truth recomputed with either operand rounded to 11 significant bits, or with the lowest set bit of both operands
    dropped (the lo x lo term of a three-product split), differs in every non-zero element of every product output: one
    wrong element fails the GPU test, and here every element is one.  The one exception is stated, not hidden: a d_x0 element
    of v2ce_convup_dgrad pools up to four taps of one gradient value, so its weights have 11 bits (four terms must sum below
    2^24) and are rounded at 10 here, and the four rounding errors of +-1 cancel in three cases of eight: more than half of
    d_x0's non-zero elements change.  The same kernel's d_x1 (12-bit weights, one term) changes everywhere."""
    kind = case[0]
    z = p1(case)[0]
    names = P.PRODUCTS[kind]
    eleven = lambda v: P.round_to_bits(v, 11)
    if kind == "updgrad" and P.is_new(case):
        # no exception here: the four terms of a d_x0 element have one sign and lose in one direction (p1w_inputs), so every
        # non-zero element changes; the 11-bit weights of the upsampled channels are rounded at 10 bits, the others at 11
        ten = lambda v: P.round_to_bits(v, 10)
        changed_everywhere(case, P.with_role(kind, z, "up", eleven), names, "up at 11 bits")
        changed_everywhere(case, P.with_role(kind, z, "other", eleven), ("x1",), "other at 11 bits")
        changed_everywhere(case, P.with_role(kind, z, "other", ten), ("x0",), "other at 10 bits")
        changed_everywhere(case, P.with_role(kind, z, "both", P.drop_lowest_bit), names, "lo x lo dropped")
        return
    if kind == "updgrad":
        changed_everywhere(case, P.with_role(kind, z, "up", eleven), ("x1",), "up at 11 bits")
        changed_everywhere(case, P.with_role(kind, z, "up", eleven), ("x0",), "up at 11 bits", all_but=0.01)
        changed_everywhere(case, P.with_role(kind, z, "other", eleven), ("x1",), "other at 11 bits")
        ten = lambda v: P.round_to_bits(v, 10)
        changed_everywhere(case, P.with_role(kind, z, "other", ten), ("x0",), "other at 10 bits", all_but=0.5)
        changed_everywhere(case, P.with_role(kind, z, "both", P.drop_lowest_bit), ("x1",), "lo x lo dropped")
        changed_everywhere(case, P.with_role(kind, z, "both", P.drop_lowest_bit), ("x0",), "lo x lo dropped", all_but=0.01)
        return
    changed_everywhere(case, P.with_role(kind, z, "up", eleven), names, "up at 11 bits")
    changed_everywhere(case, P.with_role(kind, z, "other", eleven), names, "other at 11 bits")     # (the head: feat and weight)
    changed_everywhere(case, P.with_role(kind, z, "both", P.drop_lowest_bit), names, "lo x lo dropped")


def test_wide_integer_positions_meet_the_first_tile_a_ragged_last_tile_and_a_frame_corner():
    B, L, H, W = P.P1_SHAPE
    slots = P.p1_slots()
    assert len(set(slots)) == 66 and all(b < B and l < L and h < H and w < W for b, l, h, w in slots)
    for n, of in ((16, None), (20, None), (32, None), (64, None), (32, [i for i in range(66) if (i // 2) % 2 == 0])):
        pick = P.p1_pick(n, of)
        assert pick[0] == (0, 0, 0, 0) and pick[-1] == (1, 2, 4, 128)
    last = G.tile_of(P.P1_SHAPE, G.conv_tiles(*P.P1_SHAPE) - 1)
    assert last == (1, 2, 4, 5, 128, 131)                              # one row, three columns
    by_batch = {}
    for b, l, h, w in slots:
        by_batch.setdefault(b, []).append(w)
    assert all(min(np.diff(sorted(ws))) >= 4 for ws in by_batch.values())


NEW = P.CASES[P.N_OLD:]
NEW_IDS = [P.case_id(c) for c in NEW]


def test_the_cases_were_appended():
    """The seeds come from CASES.index: the first fifteen cases are where they were."""
    assert P.N_OLD == 15 and IDS[:15] == [
        "wgrad_32_32", "wgrad_64_64", "wgrad_64_32", "wgrad_32_64", "upwgrad_64_32_32", "upwgrad_128_64_64", "upwgrad_64_64_32",
        "upwgrad_128_32_64", "dgrad_32_32", "dgrad_64_64", "dgrad_64_32", "dgrad_32_64", "updgrad_64_32_32", "head_20", "head_32"]
    assert len(set(IDS)) == len(IDS) == 26
    assert [c for c in NEW if c[0] == "wgrad"] == [c for c in P.WGRAD_CASES if P.is_new(c)] and all(c in P.CONV_CASES for c in NEW)


@pytest.mark.parametrize("case", NEW, ids=NEW_IDS)
def test_the_appended_products_have_22_or_23_significant_bits(case):
    """Odd times odd is odd, so a product's significant bits are those of its magnitude: 2^22 <= |12 bits x 12 bits| < 2^23
    (23 bits), 2^21 <= |12 bits x 11 bits| < 2^22 (22 bits: the weights of the upsampled channels of updgrad)."""
    kind, ch = case
    z = p1(case)[0]
    span = lambda v: (float(v[v != 0].abs().min()), float(v.abs().max()))
    up = [span(z[n]) for n in P.ROLES[kind]["up"]]
    other = [span(z[n]) for n in P.ROLES[kind]["other"]]
    if kind == "updgrad":
        c0 = ch[0]
        lo, hi = span(z["weight"][:, :c0])
        assert 2 ** 10 < lo and hi < 2 ** 11 and (z["weight"][:, :c0].abs() % 4 == 1).all()
        assert (z["weight"][:, :c0].sign() == z["weight"][:, :c0, :1, :1, :1].sign()).all()       # one sign per (co, ci)
        assert 2 ** 21 <= lo * min(u[0] for u in up) and hi * max(u[1] for u in up) < 2 ** 22
        other = [span(z["weight"][:, c0:]), span(z["short"])]
    assert 2 ** 22 <= min(u[0] for u in up) * min(o[0] for o in other)
    assert max(u[1] for u in up) * max(o[1] for o in other) < 2 ** 23


def test_the_appended_slot_tables_hold_disjoint_neighbourhoods_and_ragged_tiles():
    B, L, H, W = P.P1W_SHAPE
    assert G.conv_tiles(*P.P1W_SHAPE) == 72
    assert G.tile_of(P.P1W_SHAPE, 71) == (1, 3, 4, 5, 128, 131)         # the last tile: one row, three columns
    for kind, n in (("wgrad", 1760), ("dgrad", 352), ("updgrad", 264)):
        slots = P.p1w_slots(kind)
        assert len(set(slots)) == len(slots) == n and all(b < B and l < L and h < H and w < W for b, l, h, w in slots)
        assert slots[0] == (0, 0, 0, 0) and slots[-1][:2] == (1, 3) and slots[-1][3] >= 128
    assert P.p1w_slots("wgrad")[-1] == (1, 3, 4, 129)
    # the largest and the smallest slot number within a tap of every position (0 and n + 1 where there is none)
    F = torch.nn.functional
    for kind in ("dgrad", "updgrad"):
        slots = P.p1w_slots(kind)
        ids = torch.zeros((B, 1, L, H, W))
        for i, (b, l, h, w) in enumerate(slots):
            ids[b, 0, l, h, w] = i + 1
        most = F.max_pool3d(ids, 3, 1, 1)
        least = -F.max_pool3d(-torch.where(ids > 0, ids, torch.full_like(ids, len(slots) + 1.0)), 3, 1, 1)
        if kind == "updgrad":                                          # ... of every 2 x 2 pool of output positions
            most, least = F.max_pool3d(most, (1, 2, 2), ceil_mode=True), -F.max_pool3d(-least, (1, 2, 2), ceil_mode=True)
        assert ((most == 0) | (most == least)).all() and (most > 0).any(), kind
    ids = torch.zeros((B, 1, L, H, W))                                 # (and the check can fail: every third column under the pool)
    for i, (b, l, h, w) in enumerate(P.p1w_slots("dgrad")):
        ids[b, 0, l, h, w] = i + 1
    most = F.max_pool3d(F.max_pool3d(ids, 3, 1, 1), (1, 2, 2), ceil_mode=True)
    least = -F.max_pool3d(F.max_pool3d(-torch.where(ids > 0, ids, torch.full_like(ids, 353.0)), 3, 1, 1), (1, 2, 2), ceil_mode=True)
    assert ((most > 0) & (most != least)).any()
    for kind, n in (("wgrad", 32), ("wgrad", 128), ("wgrad", 512), ("dgrad", 16), ("dgrad", 64), ("dgrad", 256),
                    ("updgrad", 64), ("updgrad", 128)):
        at, later = P.p1w_pick(kind, n)
        assert len(set(at)) == n and at[0] == (0, 0, 0, 0) and at[-1] == P.p1w_slots(kind)[-1]
        assert max(w for _, _, _, w in at[:n // 2]) + 1 < later - 1 and min(w for _, _, _, w in at[n // 2:]) == later


@pytest.mark.parametrize("case", [c for c in NEW if c[0] == "updgrad"], ids=[P.case_id(c) for c in NEW if c[0] == "updgrad"])
def test_the_truth_of_the_appended_upsample_cases_is_the_numpy_restatement(case):
    """grad_probe_ref.updgrad_truth against convupn_dgrad_ref.dgrad (which torch's f64 autograd validates), and at
    (64, 32, 32) against grad_walk_ref.convup_dgrad."""
    from tests import convupn_dgrad_ref as RD
    c0, c1, cout = case[1]
    z = RD.inputs((2, 3, 5, 7), c0, c1, cout)
    want = RD.truth((2, 3, 5, 7), c0, c1, cout)
    got = P.updgrad_truth(c0, *(torch.from_numpy(z[k].copy()) for k in ("kw", "ks", "g1", "gd")))
    for k in ("d_x0", "d_x1", "abs_x0", "abs_x1"):
        assert got[k].shape == want[k].shape
        assert np.allclose(got[k].numpy(), want[k], rtol=1e-12, atol=1e-12), k
    zo = RD.inputs((2, 3, 5, 7), *RU.OLD)
    args = [torch.from_numpy(zo[k].copy()) for k in ("kw", "ks", "g1", "gd")]
    old, mine = G.convup_dgrad(*args), P.updgrad_truth(64, *args)
    assert all(torch.equal(old[k], mine[k]) for k in mine)


# ---------------------------------------------------------------------------------------------------------------------
# probe 2

N2 = int(np.prod(P.P2_SHAPE))
TILES2 = G.conv_tiles(*P.P2_SHAPE)


@pytest.mark.parametrize("case", P.WGRAD_CASES, ids=[P.case_id(c) for c in P.WGRAD_CASES])
def test_share_arithmetic_is_the_headers(case):
    kind, ch = case
    assert TILES2 == 104 and N2 == 13312
    for tiles in (1, 54, 104, 396, 1710):
        for n in (0, 1, 3, 12, 97, 300):
            mine = P.wgrad_shares(kind, ch, tiles, n)
            if kind == "wgrad":
                assert mine == R.wgrad_shares(ch[0], ch[1], tiles, n)
                if ch == (32, 32):
                    assert mine == min(tiles, G.CAP_CONV32 if n == 0 else min(G.CAP_CONV32, n))
            else:
                assert mine == RU.shares(*ch, tiles, n)
                if ch == RU.OLD:
                    assert mine == min(tiles, G.CAP_UPWGRAD_SHARES if n == 0 else min(G.CAP_UPWGRAD_SHARES, max(n // 3, 1)))
    pairs = P.pairs_of(kind, ch)
    assert P.wgrad_shares(kind, ch, TILES2, pairs) == 1 and P.share_positions(kind, ch, P.P2_SHAPE, pairs) == N2
    sizes = G.share_sizes(TILES2, P.wgrad_shares(kind, ch, TILES2))
    assert sum(sizes) == TILES2 and P.share_positions(kind, ch, P.P2_SHAPE, 0) == sizes[0] * 128
    if pairs == P.CAP:                                                 # 512 -> 512: the default grid is the one share
        assert sizes == [TILES2] and kind == "wgrad" and ch == (512, 512)
    else:
        assert sizes[0] * 128 <= hip.WGRAD_CHAIN


def test_the_walk_of_probe_2_is_three_whole_chains_and_eight_tiles():
    assert hip.WGRAD_CHAIN == hip.UPWGRAD_CHAIN == 4096
    assert divmod(TILES2, hip.WGRAD_CHAIN // 128) == (3, 8)
    assert P.P2_SHAPE[2] % G.TILE_H == 0 and P.P2_SHAPE[3] % G.TILE_W == 0


# the centre tap of an element in the anchor's row: every position is a term, the anchor's is the first
def centre_products(anchor):
    p = np.ones(N2)
    p[0] = anchor
    return p


ONE_SHARE = [(0, N2)]
DEFAULT_GRID = P.boundaries(G.share_sizes(TILES2, min(TILES2, 256)))        # v2ce_conv32_wgrad: one tile a share


def passes(assertion, grid=DEFAULT_GRID, **kernel):
    """Does the modelled kernel pass the named assertion of probe 2?  grid: the shares of the default grid."""
    if assertion == "a: header bound, one share, anchor 2^24":
        p = centre_products(2.0 ** 24)
        got = P.model_element(p, ONE_SHARE, **kernel)
        return abs(float(got) - p.sum()) <= float(P.header_bound(p.sum(), p.sum(), N2, hip.WGRAD_CHAIN))
    if assertion == "b: share bound, default grid, anchor 2^32":
        p = centre_products(2.0 ** 32)
        got = P.model_element(p, grid, **kernel)
        return abs(float(got) - p.sum()) <= float(P.share_bound(p.sum(), min(grid[0][1], hip.WGRAD_CHAIN)))
    if assertion == "b: share bound, one share, anchor 2^36":
        p = centre_products(2.0 ** 36)
        got = P.model_element(p, ONE_SHARE, **kernel)
        return abs(float(got) - p.sum()) <= float(P.share_bound(p.sum(), hip.WGRAD_CHAIN))
    assert assertion == "c: f64-throughout outputs are the exact sum rounded once"
    ok = True
    for anchor, shares in ((2.0 ** 24, ONE_SHARE), (2.0 ** 32, grid), (2.0 ** 36, ONE_SHARE)):
        p = centre_products(anchor)
        ok = ok and P.is_round32(P.model_element(p, shares, **kernel), p.sum())
    return ok


ASSERTIONS = ("a: header bound, one share, anchor 2^24", "b: share bound, default grid, anchor 2^32",
              "b: share bound, one share, anchor 2^36")
CONTRACT = dict(chain=4096, acc=np.float32, partial=np.float64, finish=np.float64)
FAULTS = {"chain of 33 tiles": (dict(CONTRACT, chain=33 * 128), ASSERTIONS[0]),
          "chain of 64 tiles": (dict(CONTRACT, chain=64 * 128), ASSERTIONS[0]),
          "no flush at all": (dict(CONTRACT, chain=None), ASSERTIONS[0]),
          "f32 partial slots": (dict(CONTRACT, partial=np.float32), ASSERTIONS[2]),
          "f32 finish": (dict(CONTRACT, finish=np.float32), ASSERTIONS[1])}


def test_the_contract_kernel_passes_every_assertion_of_probe_2():
    for a in ASSERTIONS:
        assert passes(a, **CONTRACT), a
    # the f64-throughout outputs (d_shift, d_short_bias, the head): no f32 chain at all
    assert passes("c: f64-throughout outputs are the exact sum rounded once", chain=None, acc=np.float64)
    # and the probe is live: the contract's kernel does lose the chain beside the anchor, and no more than the chain
    p = centre_products(2.0 ** 24)
    loss = p.sum() - float(P.model_element(p, ONE_SHARE, **CONTRACT))
    assert loss == 4095.0                                              # 4095 ties to even; the sum itself is an f32


@pytest.mark.parametrize("fault", FAULTS)
def test_each_faulty_kernel_fails_the_assertion_named_for_it(fault):
    kernel, caught_by = FAULTS[fault]
    assert not passes(caught_by, **kernel), (fault, caught_by)


# the default grids of the appended weight-gradient cases: 16 pairs (128 -> 128, 512 -> 32, 32 -> 512) give 16 shares of 6 or 7
# tiles, 256 pairs (512 -> 512) the one share
WIDE_GRIDS = {p: P.boundaries(G.share_sizes(TILES2, min(TILES2, P.CAP // p))) for p in (16, 256)}


def test_the_grids_of_the_appended_cases_are_the_modelled_ones():
    want = {P.pairs_of(*c) for c in P.WGRAD_CASES if P.is_new(c)}
    assert want == set(WIDE_GRIDS) and len(WIDE_GRIDS[16]) == 16 and WIDE_GRIDS[256] == ONE_SHARE
    for c in (c for c in P.WGRAD_CASES if P.is_new(c)):
        assert WIDE_GRIDS[P.pairs_of(*c)][0][1] == P.share_positions(*c, P.P2_SHAPE, 0)


@pytest.mark.parametrize("pairs", WIDE_GRIDS)
def test_at_the_appended_pair_counts_each_fault_breaks_an_assertion(pairs):
    """A 64-tile chain breaks (a) and an f32 partial slot breaks (b) at one share, whatever the pair count.  An f32 finish
    breaks (b) at the default grid of 16 pairs; at 256 pairs the default grid is one share, the finish adds one slot to
    zero, and an f32 finish is the contract's kernel byte for byte: there is nothing to catch."""
    grid = WIDE_GRIDS[pairs]
    for a in ASSERTIONS:
        assert passes(a, grid, **CONTRACT), a
    assert not passes(ASSERTIONS[0], grid, **dict(CONTRACT, chain=64 * 128))
    assert not passes(ASSERTIONS[2], grid, **dict(CONTRACT, partial=np.float32))
    f32_finish = dict(CONTRACT, finish=np.float32)
    if pairs == 256:
        for anchor in (2.0 ** 24, 2.0 ** 32, 2.0 ** 36):
            p = centre_products(anchor)
            assert P.model_element(p, grid, **f32_finish) == P.model_element(p, grid, **CONTRACT)
        # the chain is what the default grid's anchor of 2^32 sees there: a 64-tile chain breaks (b) as well
        assert not passes(ASSERTIONS[1], grid, **dict(CONTRACT, chain=64 * 128))
    else:
        assert not passes(ASSERTIONS[1], grid, **f32_finish)


def test_an_f32_accumulator_fails_the_exactness_of_the_f64_throughout_outputs():
    assert not passes("c: f64-throughout outputs are the exact sum rounded once", chain=None, acc=np.float32)
    assert not passes("c: f64-throughout outputs are the exact sum rounded once", **CONTRACT)


def test_the_bound_of_probe_2a_sits_between_the_chain_and_a_chain_of_33_tiles():
    s = 2.0 ** 24 + N2 - 1
    b = float(P.header_bound(s, s, N2, hip.WGRAD_CHAIN))
    assert hip.WGRAD_CHAIN < b < 33 * 128 - 1 and 4100 < b < 4102


def test_the_anchors_of_probe_2_are_where_the_docstring_says():
    for case in P.WGRAD_CASES:
        kind, ch = case
        for where in ("up", "input"):
            z = P.p2_inputs(case, 2.0 ** 24, where)
            hit = {k: (v == 2.0 ** 24).nonzero().tolist() for k, v in z.items() if v is not None}
            assert all(((v == 1) | (v == 2.0 ** 24)).all() for v in z.values() if v is not None)
            if where == "up":
                want = [[0, c, 0, 0, 0] for c in range(P.P2_UP_CHANNEL, ch[-1], 32)]
                assert all(hit[k] == want for k in P.ROLES[kind]["up"]) and not any(hit[k] for k in P.ROLES[kind]["other"])
            elif kind == "wgrad":
                assert hit["x"] == [[0, c, 1, 14, 30] for c in range(P.P2_IN_CHANNEL, ch[0], 32)] and not hit["upstream"]
            else:
                assert hit["x1"] == [[0, 7, 1, 14, 30]] and hit["x0"] == [[0, 9, 1, 7, 15]] and not hit["g1"] and not hit["gd"]


# ---------------------------------------------------------------------------------------------------------------------
# probe 3

@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_scaled_normals_stay_inside_the_normal_range(case):
    """No |value|, no |product of paired values| and no |truth| of the plain data lies outside [2^-60, 2^40]; with exponents
    of at most 16 on both operands nothing then leaves f32's normal range, and the scaling commutes with every rounding."""
    kind = case[0]
    z = P.normal_inputs(case, P.p3_shape(case), P.P3_SEED)
    lo, hi = P.P3_RANGE
    span = {}
    for role in ("up", "other"):
        a = torch.cat([z[n].abs().reshape(-1) for n in P.ROLES[kind][role]])
        span[role] = (float(a.min()), float(a.max()))
        assert lo <= span[role][0] and span[role][1] <= hi, (case, role, span[role])
    assert lo <= span["up"][0] * span["other"][0] and span["up"][1] * span["other"][1] <= hi, (case, span)
    t = P.truth(kind, z, case[1])
    for name in P.OUTPUTS[kind]:
        a = t[name].abs()
        a = a[a != 0] if name == "res" else a                          # d_res is a copy: the mask's zeros are zeros
        assert lo <= float(a.min()) and float(a.max()) <= hi, (case, name, float(a.min()), float(a.max()))
    for name in P.ROLES[kind]["up"] + P.ROLES[kind]["other"]:
        e = P.exponents(case, name, 192)
        assert int(e.abs().max()) <= P.P3_MAX_EXP and len(set(e.tolist())) > 8
