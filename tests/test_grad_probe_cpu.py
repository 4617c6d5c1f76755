"""CPU side of the probe tests of the eight gradient kernels (tests/test_gpu_grad_probes.py): the conditions on the data of
probes 1 and 3 that make their bit-exact assertions valid and sharp, the share arithmetic of probe 2 against the headers'
host-side restatements, and a numpy model of hypothetical weight-gradient kernels (tests/grad_probe_ref.py: model_element)
showing that the contract's kernel passes every assertion of probe 2 and that each faulty variant fails a named one.

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
    return z, P.truth(case[0], z)


def changed_everywhere(case, z2, names, label, all_but=0.0):
    """Every non-zero element of the named outputs (all but the fraction `all_but`) differs between the truth and the truth of
    the altered inputs z2."""
    t, t2 = p1(case)[1], P.truth(case[0], z2)
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
    a = P.abs_truth(kind, z)
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


def passes(assertion, **kernel):
    """Does the modelled kernel pass the named assertion of probe 2?"""
    if assertion == "a: header bound, one share, anchor 2^24":
        p = centre_products(2.0 ** 24)
        got = P.model_element(p, ONE_SHARE, **kernel)
        return abs(float(got) - p.sum()) <= float(P.header_bound(p.sum(), p.sum(), N2, hip.WGRAD_CHAIN))
    if assertion == "b: share bound, default grid, anchor 2^32":
        p = centre_products(2.0 ** 32)
        got = P.model_element(p, DEFAULT_GRID, **kernel)
        return abs(float(got) - p.sum()) <= float(P.share_bound(p.sum(), 128))
    if assertion == "b: share bound, one share, anchor 2^36":
        p = centre_products(2.0 ** 36)
        got = P.model_element(p, ONE_SHARE, **kernel)
        return abs(float(got) - p.sum()) <= float(P.share_bound(p.sum(), hip.WGRAD_CHAIN))
    assert assertion == "c: f64-throughout outputs are the exact sum rounded once"
    ok = True
    for anchor, shares in ((2.0 ** 24, ONE_SHARE), (2.0 ** 32, DEFAULT_GRID), (2.0 ** 36, ONE_SHARE)):
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
    z = P.normal_inputs(case, P.P3_SHAPE, P.P3_SEED)
    lo, hi = P.P3_RANGE
    span = {}
    for role in ("up", "other"):
        a = torch.cat([z[n].abs().reshape(-1) for n in P.ROLES[kind][role]])
        span[role] = (float(a.min()), float(a.max()))
        assert lo <= span[role][0] and span[role][1] <= hi, (case, role, span[role])
    assert lo <= span["up"][0] * span["other"][0] and span["up"][1] * span["other"][1] <= hi, (case, span)
    t = P.truth(kind, z)
    for name in P.OUTPUTS[kind]:
        a = t[name].abs()
        a = a[a != 0] if name == "res" else a                          # d_res is a copy: the mask's zeros are zeros
        assert lo <= float(a.min()) and float(a.max()) <= hi, (case, name, float(a.min()), float(a.max()))
    for name in P.ROLES[kind]["up"] + P.ROLES[kind]["other"]:
        e = P.exponents(case, name, 192)
        assert int(e.abs().max()) <= P.P3_MAX_EXP and len(set(e.tolist())) > 8
