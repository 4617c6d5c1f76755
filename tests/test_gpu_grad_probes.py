"""The precision contracts of the eleven gradient kernels on data that can see them fail: v2ce_conv32_wgrad,
v2ce_convup_wgrad, v2ce_convn_wgrad, v2ce_convupn_wgrad, v2ce_conv32_dgrad, v2ce_convup_dgrad, v2ce_convn_dgrad,
v2ce_pred_head_grads, v2ce_convc_wgrad, v2ce_convc_dgrad and v2ce_convupn_dgrad through their checked Python entries,
against the f64 truths of the suite computed on the device
(tests/grad_probe_ref.py builds the data and states the assertions; tests/test_grad_probe_cpu.py proves the data's conditions
and shows on a numpy model which assertion catches which fault).  The N-channel kernels run at convn_ref.PAIRS and
convupn_ref.TRIPLES.  The integers 1 .. 3 and the standard normals of the other tests cannot see these sentences fail.

The last three entries are the cases appended to grad_probe_ref.CASES:
  wgrad    (128, 128), (512, 32), (32, 512), (512, 512)     conv_grads.convc_wgrad (up to 256 pairs: one share by default)
  dgrad    (128, 128), (512, 32), (32, 512), (512, 512)     conv_grads.convc_dgrad (the instance that fetches weights per tile)
  updgrad  (128, 64, 64), (64, 64, 32), (128, 32, 64)       dec2_block.convupn_dgrad
with shapes of their own in probes 1 and 3: [2, 4, 5, 131] (up to 512 sparse positions, 256 with disjoint neighbourhoods;
the input gradients also at max_workgroups = 97) and [1, 3, 20, 70] (60 tiles, a ragged second tile column).

Probe 1, "exact f32 products".  [2, 3, 5, 131], sparse upstream gradients and dense operands of odd 12-bit integers: every
product has 22 or 23 significant bits, every element's sum of |terms| is below 2^24, so every output must equal the f64
truth rounded to f32 bit for bit, whatever the order of the f32 sums -- and a product formed in an 11-bit format, or a
three-product split without its lo x lo term, changes every non-zero element.  The weight gradients run at the default grid
(an element's two terms meet in f64) and at one share (they meet in one f32 chain).  Outputs go in filled with NaN.

Probe 2, "at most CHAIN positions" and "everything above that level is f64".  [1, 4, 26, 128], 104 full tiles; ones, and
one anchor.  (a) One share, an anchor of 2^24 first in the walk (in the upstream gradient) or inside tile 40 (in the input):
the 4095 ones behind the anchor in its chain are ties that round to even and are lost, everything behind the flush is kept:
the header's own bound, about 4101, holds elementwise; a chain of 33 tiles loses 4223.  The loss at the centre tap is
printed and must be positive: the anchor was absorbed, the probe is live.  (b) An anchor of 2^32 at the default grid, where
an f32 finish loses every other share, and of 2^36 at one share, where an f32 partial slot loses every other chain: the
error is at most ulp32(exact) + the positions that share the anchor's f32 chain (its share's, at most CHAIN).  (c) d_shift,
d_short_bias and the three outputs of the head (an anchor of 2^30) are f64 throughout: the exact sum rounded once.

Probe 3, per-element arithmetic.  The walks' normal data at [2, 3, 43, 131], once plain and once with every channel of every
input scaled by its own power of two: an f32 fmaf chain, an f64 sum and one rounding commute with the scaling, so the
outputs are the plain run's bytes times the powers of two (input gradients: the same bytes when the weight takes the
inverse scale).  A scale shared between channels, or a sum in a fixed-point or block-scaled format, cannot pass.

Probe 4, below the normal range.  [1, 2, 5, 70], normals scaled so that products lie around 2^-126 (both operands at 2^-64)
and so that one operand is subnormal while the products are normal (2^-130 against 2^20): the header bounds hold."""
import numpy as np
import pytest
import torch

from tests import convn_ref as R
from tests import grad_probe_ref as P
from tests import grad_walk_ref as G
from tests import last_block_dgrad_ref as BD
from tests.last_conv_ref import ulp32
from tests import convupn_ref as RU
from v2ce_toolbox_amd import conv_grads, dec2_block, dec2_conv, hip, last_block, last_conv, pred_head

pytestmark = pytest.mark.gpu

DEV = "cuda"
ids = lambda cases: [P.case_id(c) for c in cases]


def nan(shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=DEV)


def c16(a):
    return G.to_c16(a.to(DEV), G.pitch_of(a.shape[4]))


def run(case, z, shape, cap=0):
    """One call of the case's checked entry on the CPU inputs z (reference layouts) -> {name: output in the truth's layout on
    the device}.  Every output goes in filled with NaN; the padding columns of every channels-last-16 input hold NaN."""
    kind, ch = case
    B, L, H, W = shape
    kw = {"max_workgroups": cap}
    if kind == "wgrad":
        cin, cout = ch
        f = last_conv.conv32_wgrad if ch == (32, 32) else conv_grads.convc_wgrad if P.is_new(case) else dec2_conv.convn_wgrad
        g = f(c16(z["x"]), None if z["y"] is None else c16(z["y"]), c16(z["upstream"]),
              out={"weight": nan((cout, cin, 3, 3, 3)), "shift": nan((cout,))}, **kw)
    elif kind == "upwgrad":
        c0, c1, cout = ch
        f = last_block.convup_wgrad if ch == (64, 32, 32) else dec2_block.convupn_wgrad
        g = f(c16(z["x0"]), c16(z["x1"]), c16(z["g1"]), c16(z["gd"]),
              out={"weight": nan((cout, c0 + c1, 3, 3, 3)), "short": nan((cout, c0 + c1)), "short_bias": nan((cout,))}, **kw)
    elif kind == "dgrad":
        cin, cout = ch
        f = last_conv.conv32_dgrad if ch == (32, 32) else conv_grads.convc_dgrad if P.is_new(case) else dec2_conv.convn_dgrad
        up = c16(z["upstream"])
        out = {"x": nan((B, L, cin // 16, H, up.shape[4], 16)), "res": nan(up.shape)}
        for t in out.values():
            t.lw, t.c16 = W, True
        g = f(z["weight"].to(DEV), None if z["y"] is None else c16(z["y"]), up, out=out, **kw)
    elif kind == "updgrad":
        g1 = c16(z["g1"])
        x0 = nan((B, L, ch[0] // 16, (H + 1) // 2, G.pitch_of((W + 1) // 2), 16))
        f = last_block.convup_dgrad if ch == RU.OLD else dec2_block.convupn_dgrad          # (the planes of x0 say c0)
        x1 = nan((B, L, ch[1] // 16, H, g1.shape[4], 16))
        g = f(z["weight"].to(DEV), z["short"].to(DEV), g1, c16(z["gd"]), out={"x0": x0, "x1": x1}, **kw)
    else:
        assert cap == 0
        feat = c16(z["feat"])
        g = pred_head.pred_head_grads(feat, G.to_dense(z["y"].to(DEV)), G.to_dense(z["upstream"].to(DEV)), z["weight"].to(DEV),
                                      want=("weight", "bias", "feat"), out={"feat": nan(feat.shape)})
    torch.cuda.synchronize()
    assert set(g) == set(P.OUTPUTS[kind])
    out = {}
    for name, t in g.items():
        v = G.from_c16(t, (W + 1) // 2 if name == "x0" else W) if t.dim() == 6 else t
        if kind == "head" and name == "weight":
            v = v.reshape(-1, G.C)
        assert not torch.isnan(v).any(), (case, name, "NaN: an element was not written, or a padding column was read")
        out[name] = v
    return out


def device_truth(kind, z, ch=None):
    return P.truth(kind, {k: (None if v is None else v.to(DEV)) for k, v in z.items()}, ch)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def mismatch(got, want):
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
    return f"{bad.shape[0]} of {got.numel()} elements differ; first (index, got, want): {first}"


def pairs(case):
    return P.pairs_of(*case)


# ---------------------------------------------------------------------------------------------------------------------
# probe 1

@pytest.mark.parametrize("case", P.CASES, ids=ids(P.CASES))
def test_wide_integers_are_bit_exact(case):
    kind = case[0]
    z = P.p1_inputs(case)
    t = device_truth(kind, z, case[1])
    # the weight gradients also at one share; the appended input gradients also at a prime grid of uneven shares
    grids = (0, pairs(case)) if kind in ("wgrad", "upwgrad") else (0, R.PRIME_GRID) if P.is_new(case) else (0,)
    for cap in grids:
        own = run(case, z, P.p1_shape(case), cap)
        for name in P.OUTPUTS[kind]:
            want = t[name].to(torch.float32)
            assert torch.equal(want.to(torch.float64), t[name]) and (want != 0).any()
            assert same_bytes(own[name], want), (case, f"max_workgroups={cap}", name, mismatch(own[name], want))


# ---------------------------------------------------------------------------------------------------------------------
# probe 2

N2 = int(np.prod(P.P2_SHAPE))


def chain_of(case):
    return hip.WGRAD_CHAIN if case[0] == "wgrad" else hip.UPWGRAD_CHAIN


def p2(case, anchor, where, cap):
    z = P.p2_inputs(case, anchor, where)
    t = {k: v.cpu().numpy() for k, v in device_truth(case[0], z).items()}
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in run(case, z, P.P2_SHAPE, cap).items()}
    return t, got


def exact_outputs(case, t, got, label):
    for name in P.OUTPUTS[case[0]]:
        if name not in P.PRODUCTS[case[0]]:
            assert P.is_round32(got[name], t[name]), (case, label, name, got[name][:8], t[name][:8])


@pytest.mark.parametrize("where", ["up", "input"])
@pytest.mark.parametrize("case", P.WGRAD_CASES, ids=ids(P.WGRAD_CASES))
def test_one_chain_absorbs_at_most_its_own_positions(case, where):
    kind, ch = case
    t, got = p2(case, 2.0 ** 24, where, pairs(case))
    for name in P.PRODUCTS[kind]:
        err = np.abs(got[name] - t[name])                       # (every term is positive: the truth is its own sum of |terms|)
        bound = P.header_bound(t[name], t[name], N2, chain_of(case))
        centre = (t[name] - got[name])[:, :, 1, 1, 1] if name == "weight" else t[name] - got[name]
        rows = centre[P.P2_UP_CHANNEL::32] if where == "up" else centre
        print(f"probe 2a {P.case_id(case)} anchor in {where}: {name}: loss at the centre tap {float(rows.max()):.0f}, "
              f"max error {float(err.max()):.0f}, {float((err / bound).max()):.3g} of the header bound")
        assert np.all(err <= bound), (case, where, name, float(err.max()), float((err / bound).max()))
        if where == "up":
            assert 0 < rows.min() and rows.max() <= chain_of(case), (case, name, "the anchor was not absorbed: the probe is dead")
            assert 4100 < bound[P.P2_UP_CHANNEL].max() < 4102
    exact_outputs(case, t, got, where)


@pytest.mark.parametrize("grid", ["default_grid", "one_share"])
@pytest.mark.parametrize("case", P.WGRAD_CASES, ids=ids(P.WGRAD_CASES))
def test_everything_above_the_chain_is_f64(case, grid):
    kind, ch = case
    anchor, cap = (2.0 ** 32, 0) if grid == "default_grid" else (2.0 ** 36, pairs(case))
    # share_positions knows the grids: at 512 -> 512 (256 pairs) the default grid is itself the one share of 104 tiles, so
    # both parametrisations walk the same grid there, with their two anchors, and the chain is what bounds the positions
    positions = min(P.share_positions(kind, ch, P.P2_SHAPE, cap), chain_of(case))
    assert positions == (chain_of(case) if cap or pairs(case) == P.CAP else P.share_positions(kind, ch, P.P2_SHAPE, 0))
    t, got = p2(case, anchor, "up", cap)
    for name in P.PRODUCTS[kind]:
        err = np.abs(got[name] - t[name])
        bound = P.share_bound(t[name], positions)
        print(f"probe 2b {P.case_id(case)} {grid}: {name}: max error {float(err.max()):.0f}, bound {float(bound.max()):.0f} "
              f"({positions} positions beside the anchor)")
        assert np.all(err <= bound), (case, grid, name, float(err.max()), float(bound.max()))
    exact_outputs(case, t, got, grid)


@pytest.mark.parametrize("cout", G.HEAD_COUTS)
def test_the_head_is_f64_throughout(cout):
    case = ("head", (cout,))
    z = P.p2_inputs(case, P.HEAD_ANCHOR, "up")
    t = {k: v.cpu().numpy() for k, v in device_truth("head", z).items()}
    got = run(case, z, P.P2_SHAPE)
    assert t["weight"][3, 0] == P.HEAD_ANCHOR + N2 - 1 and t["bias"][3] == P.HEAD_ANCHOR + N2 - 1
    for name in P.OUTPUTS["head"]:
        assert P.is_round32(got[name].cpu().numpy(), t[name]), (cout, name)


# ---------------------------------------------------------------------------------------------------------------------
# probe 3

def ex(case, name, n):
    return P.exponents(case, name, n).to(DEV)


def expect(case, label, name, got, plain, exps=None):
    """got must be the plain run's bytes, times 2^exps (which broadcasts against the output)."""
    want = plain if exps is None else plain * P.pow2(exps)
    assert torch.isfinite(want).all() and ((want == 0) | (want.abs() >= 2.0 ** -126)).all()
    assert same_bytes(got, want), (case, label, name, mismatch(got, want))


def col(e, dims_behind):
    return e.view([-1] + [1] * dims_behind)


@pytest.mark.parametrize("case", P.CASES, ids=ids(P.CASES))
def test_a_power_of_two_per_channel_scales_every_output_exactly(case):
    kind, ch = case
    shape = P.p3_shape(case)
    z = P.normal_inputs(case, shape, P.P3_SEED)
    plain = run(case, z, shape)
    sc = lambda name, e, dim: P.scaled(z[name], e.cpu(), dim)
    if kind == "wgrad":
        a, b = ex(case, "x", ch[0]), ex(case, "upstream", ch[1])
        own = run(case, dict(z, x=sc("x", a, 1), upstream=sc("upstream", b, 1)), shape)
        expect(case, "a, b", "weight", own["weight"], plain["weight"], col(b, 4) + col(a, 3))
        expect(case, "a, b", "shift", own["shift"], plain["shift"], b)
    elif kind == "upwgrad":
        c0, c1, cout = ch
        a, b1, bd = ex(case, "x", c0 + c1), ex(case, "g1", cout), ex(case, "gd", cout)
        own = run(case, dict(z, x0=sc("x0", a[:c0], 1), x1=sc("x1", a[c0:], 1), g1=sc("g1", b1, 1), gd=sc("gd", bd, 1)), shape)
        expect(case, "a, b", "weight", own["weight"], plain["weight"], col(b1, 4) + col(a, 3))
        expect(case, "a, b", "short", own["short"], plain["short"], col(bd, 1) + a)
        expect(case, "a, b", "short_bias", own["short_bias"], plain["short_bias"], bd)
    elif kind == "dgrad":
        a, b = ex(case, "x", ch[0]), ex(case, "upstream", ch[1])
        own = run(case, dict(z, upstream=sc("upstream", b, 1), weight=sc("weight", -b, 0)), shape)
        expect(case, "b against 1 / b", "x", own["x"], plain["x"])                       # the products are the same numbers
        want_res = plain["res"] * P.pow2(col(b, 3))
        assert same_bytes(own["res"], want_res), (case, "res is a copy", mismatch(own["res"], want_res))
        own = run(case, dict(z, weight=sc("weight", a, 1)), shape)
        expect(case, "a", "x", own["x"], plain["x"], col(a, 3))
        assert same_bytes(own["res"], plain["res"]), (case, "res is a copy")
    elif kind == "updgrad":
        c0, c1, cout = ch
        a, b1, bd = ex(case, "x", c0 + c1), ex(case, "g1", cout), ex(case, "gd", cout)
        own = run(case, dict(z, g1=sc("g1", b1, 1), weight=sc("weight", -b1, 0), gd=sc("gd", bd, 1), short=sc("short", -bd, 0)),
                  shape)
        for name in ("x0", "x1"):
            expect(case, "b against 1 / b", name, own[name], plain[name])
        own = run(case, dict(z, weight=sc("weight", a, 1), short=sc("short", a, 1)), shape)
        expect(case, "a", "x0", own["x0"], plain["x0"], col(a[:c0], 3))
        expect(case, "a", "x1", own["x1"], plain["x1"], col(a[c0:], 3))
    else:
        a, b = ex(case, "feat", G.C), ex(case, "upstream", ch[0])
        own = run(case, dict(z, feat=sc("feat", a, 1), upstream=sc("upstream", b, 1), weight=sc("weight", -b, 0)), shape)
        expect(case, "a, b", "weight", own["weight"], plain["weight"], col(b, 1) + a)
        expect(case, "a, b", "bias", own["bias"], plain["bias"], b)
        expect(case, "b against 1 / b", "feat", own["feat"], plain["feat"])
        own = run(case, dict(z, weight=sc("weight", a, 1)), shape)
        expect(case, "a", "feat", own["feat"], plain["feat"], col(a, 3))


# ---------------------------------------------------------------------------------------------------------------------
# probe 4

P4_SCALES = {"products_around_2^-126": (-64, -64), "subnormal_gradient": (-130, 20), "subnormal_operand": (20, -130)}


def report(label, name, err, bound):
    frac = float((err / bound).max())
    print(f"{label}: {name}: max error {float(err.max()):.3e}, {frac:.3g} of its bound")
    assert np.all(err <= bound), (label, name, float(err.max()), frac)


@pytest.mark.parametrize("scales", P4_SCALES)
@pytest.mark.parametrize("case", P.CONV_CASES, ids=ids(P.CONV_CASES))
def test_the_header_bounds_hold_below_the_normal_range(case, scales):
    kind, ch = case
    e_up, e_other = P4_SCALES[scales]
    z = P.normal_inputs(case, P.P4_SHAPE, P.P4_SEED)
    half = lambda v, e: v * 2.0 ** (e // 2) * 2.0 ** (e - e // 2)          # (2^-130 is not a normal f32: two exact steps)
    z = {k: (v if k == "y" else half(v, e_up if k in P.ROLES[kind]["up"] else e_other)) for k, v in z.items()}
    if e_up == -130:
        assert all((z[k].abs() < 2.0 ** -126).all() and (z[k] != 0).float().mean() > 0.9 for k in P.ROLES[kind]["up"])
    t = {k: v.cpu().numpy() for k, v in device_truth(kind, z, ch).items()}
    s = {k: v.cpu().numpy() for k, v in P.abs_truth(kind, {k: (None if v is None else v.to(DEV)) for k, v in z.items()}, ch).items()}
    got = {k: v.cpu().numpy() for k, v in run(case, z, P.P4_SHAPE).items()}
    n = int(np.prod(P.P4_SHAPE))
    label = f"probe 4 {P.case_id(case)} {scales}"
    err = lambda name: np.abs(got[name].astype(np.float64) - t[name])
    for name in P.OUTPUTS[kind]:
        live = float(np.mean(got[name] != 0))
        print(f"{label}: {name}: {live:.3f} of the elements are not zero, max |exact| {float(np.abs(t[name]).max()):.3e}")
    if kind in ("wgrad", "upwgrad"):
        chain = hip.WGRAD_CHAIN if kind == "wgrad" else hip.UPWGRAD_CHAIN
        for name in P.PRODUCTS[kind]:
            report(label, name, err(name), R.wgrad_bound(t[name], s[name], n, chain))
        for name in set(P.OUTPUTS[kind]) - set(P.PRODUCTS[kind]):                        # f64 throughout: one rounding
            rounded = t[name].astype(np.float32).astype(np.float64)
            report(label, name, np.abs(got[name].astype(np.float64) - rounded), ulp32(t[name]))
    elif kind == "dgrad":
        report(label, "x", err("x"), R.dgrad_bound(s["x"], ch[1]))
        assert np.array_equal(got["res"].view(np.int32), t["res"].astype(np.float32).view(np.int32)), (label, "res is a copy")
    else:
        terms = hip.UPDGRAD_TERMS if ch == RU.OLD else hip.UPNDGRAD_TERMS(ch[2])
        report(label, "x1", err("x1"), BD.dgrad_bound(s["x1"], terms))
        report(label, "x0", err("x0"), BD.dgrad_bound(s["x0"], terms * P.n_terms_updgrad(P.P4_SHAPE)))
