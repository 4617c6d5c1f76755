"""v2ce_convupn_dgrad (include/v2ce_hip_convupndgrad.h) through its checked Python entry (dec2_block.convupn_dgrad) on the
GPU against the numpy f64 restatement of the header's formulas (tests/convupn_dgrad_ref.py, which
tests/test_convupn_dgrad_cpu.py ties to torch's f64 autograd), in the scheme of tests/test_gpu_convupdgrad.py.

Bound (from the header's precision contract, not from what the kernel gives), plus one ulp of the truth for its rounding:
  d_x1  |err| <= (n + 1) 2^-24 abs_terms + n 2^-126 with n = V2CE_UPNDGRAD_TERMS(cout) = 28 cout: an f32 sum of n exact
        products in some fixed order (abs_terms = the f64 sum of |terms| of the element), and what is flushed below the
        normal range;
  d_x0  the same with n = 28 cout times the number of output positions of the source pixel (1, 2 or 4).
On the integer data of tests/convupn_dgrad_ref.py every sum is exact (tests/test_convupn_dgrad_cpu.py shows the margin), so
there the kernel equals the truth at zero tolerance, whatever its order of summation.
Every tensor goes in at pitch = W + 3 and pitch0 = W0 + 5 with NaN in the inputs' padding columns and NaN all over the
outputs.  Every result is printed as a fraction of its bound."""
import numpy as np
import pytest
import torch

from tests import convupn_dgrad_ref as R
from v2ce_toolbox_amd import dec2_block, last_block

pytestmark = pytest.mark.gpu

DEC2 = R.DEC2
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 3, 70), (1, 2, 4, 65), (1, 3, 6, 64)]
BIG = (1, 3, 20, 70)
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def offset_copy(a, elems):
    """A device copy of `a` whose first element sits `elems` floats past an allocation's start."""
    a = np.ascontiguousarray(a, np.float32)
    flat = torch.zeros(a.size + elems + 64, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 256 == 0
    v = flat[elems:elems + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def device(a, shifted=False):
    """[B, C, L, H, W] -> the kernel's channels-last-16 tensor at pitch W + 3, padding columns NaN; shifted: the base
    pointer 16 bytes past a 256-byte boundary."""
    W = a.shape[-1]
    t = offset_copy(R.to_c16(a, W + 3), 4 if shifted else 0)
    t.lw, t.c16 = W, True
    return t


def run(tr, z, g1=True, gd=True, shifted=False, want=("x0", "x1"), arrays=None, entry=None, **kw):
    """-> {name: the whole channels-last-16 output as numpy, padding columns included}."""
    c0, c1, cout = tr
    a1, ad = arrays if arrays is not None else (z["g1"], z["gd"])
    B, _, L, H, W = a1.shape
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    shape = {"x0": (B, L, c0 // 16, H0, W0 + 5, 16), "x1": (B, L, c1 // 16, H, W + 3, 16)}
    out = {n: offset_copy(np.full(shape[n], np.nan, np.float32), 4 if shifted else 0) for n in want}
    w, s = torch.from_numpy(z["kw"].copy()).cuda(), torch.from_numpy(z["ks"].copy()).cuda()
    if entry is None:
        entry = dec2_block.convupn_dgrad
        if "x0" not in want:
            kw["c0"] = c0                             # (128 input channels do not say how they split)
    g = entry(w if g1 else None, s if gd else None, device(a1, shifted) if g1 else None, device(ad, shifted) if gd else None,
              want=want, out=out, **kw)
    torch.cuda.synchronize()
    assert set(g) == set(want)
    for n, t in g.items():
        assert t is out[n] and t.lw == (W0 if n == "x0" else W) and t.c16
    return {k: v.cpu().numpy() for k, v in g.items()}


def logical(got, W):
    """{name: [B, C, L, h, w] f64 of the logical columns}; asserts that nothing of the NaN fill or padding is left and that
    the padding columns are exact zeros."""
    res = {}
    for k, a in got.items():
        lw = (W + 1) // 2 if k == "x0" else W
        assert not np.isnan(a).any(), k
        assert not a[:, :, :, :, lw:, :].any(), k
        res[k] = R.from_c16(a, lw).astype(np.float64)
    return res


def check(got, tr, t, label):
    W = t["d_x1"].shape[-1]
    vals, b = logical(got, W), R.bounds(tr[2], t["abs_x0"], t["abs_x1"])
    for k, v in vals.items():
        truth = t[f"d_{k}"]
        err, bound = np.abs(v - truth), b[k] + R.ulp32(truth)
        print(f"{label}: d_{k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound")
        assert v.shape == truth.shape and np.all(err <= bound), (label, k, float(err.max()))


@pytest.mark.parametrize("shape", SHAPES + ["zero"], ids=ids)
def test_dec2_triple_matches_the_f64_truth(shape):
    kind, shape = ("zero", (2, 3, 5, 7)) if shape == "zero" else ("normal", shape)
    z, t = R.inputs(shape, *DEC2, kind), R.truth(shape, *DEC2, kind)
    got = run(DEC2, z)
    check(got, DEC2, t, f"128+64->64 {ids(shape)} {kind}")
    if kind == "zero":
        assert not got["x0"].any() and not got["x1"].any()
    else:
        assert np.abs(t["d_x0"]).max() > 0 and np.abs(t["d_x1"]).max() > 0
    if shape == (1, 2, 4, 65):
        # the last tile is one column wide: source column 32 collects output column 64 alone
        v = logical(got, 65)
        want = t["d_X"][:, :128, :, 0::2, 64] + t["d_X"][:, :128, :, 1::2, 64]
        b = R.bounds(64, t["abs_x0"], t["abs_x1"])["x0"]
        assert np.all(np.abs(v["x0"][..., 32] - want) <= b[..., 32] + R.ulp32(want))
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("tr", [tr for tr in R.TRIPLES if tr != DEC2], ids=ids)
def test_the_other_triples_match_the_f64_truth(tr):
    shape = (2, 3, 5, 7)
    check(run(tr, R.inputs(shape, *tr)), tr, R.truth(shape, *tr), f"{ids(tr)} {ids(shape)}")


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 3, 70)], ids=ids)
@pytest.mark.parametrize("tr", [DEC2, (128, 32, 64)], ids=ids)
def test_integer_data_bit_for_bit(tr, shape):
    """Every product and partial sum is an integer below 2^24: the kernel's f32 sums are exact in any order, so a wrong
    plane, co group or X-group index cannot hide behind a tolerance."""
    z, t = R.inputs(shape, *tr, "int", 5), R.truth(shape, *tr, "int", 5)
    got = run(tr, z)
    v = logical(got, shape[3])
    for k in ("x0", "x1"):
        assert np.array_equal(v[k], t[f"d_{k}"]), (k, float(np.abs(v[k] - t[f"d_{k}"]).max()))
        assert np.abs(t[f"d_{k}"]).max() > 0
    # the second co group really enters: without the channels 32 .. 63 of g1 both outputs change
    g1 = z["g1"].copy()
    g1[:, 32:] = 0
    other = logical(run(tr, z, arrays=(g1, z["gd"])), shape[3])
    half = R.dgrad(*tr, z["kw"], z["ks"], g1, z["gd"])
    for k in ("x0", "x1"):
        assert np.array_equal(other[k], half[f"d_{k}"]) and not np.array_equal(other[k], v[k]), k


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 4, 65), BIG], ids=ids)
def test_64_32_32_gives_the_bytes_of_the_older_entry(shape):
    z = R.inputs(shape, *R.OLD)
    new, old = run(R.OLD, z), run(R.OLD, z, entry=last_block.convup_dgrad)
    assert new["x0"].tobytes() == old["x0"].tobytes() and new["x1"].tobytes() == old["x1"].tobytes()
    assert np.abs(new["x0"]).max() > 0 and np.abs(new["x1"]).max() > 0
    if shape == BIG:
        capped = run(R.OLD, z, max_workgroups=3)
        assert capped["x0"].tobytes() == old["x0"].tobytes() and capped["x1"].tobytes() == old["x1"].tobytes()


def test_shares_add_up():
    """The g1-only call plus the gd-only call is the combined call: each of the three is within its own bound of its exact
    value, and the exact values add up, so the difference is within the sum of the three bounds (plus the f64 rounding of
    the test's own addition, a 2^-52 relative term that an ulp32 covers)."""
    shape = (2, 3, 5, 7)
    z, tb = R.inputs(shape, *DEC2), R.truth(shape, *DEC2)
    both, conv, short = run(DEC2, z), run(DEC2, z, gd=False), run(DEC2, z, g1=False)
    vb, vc, vs = (logical(g, 7) for g in (both, conv, short))
    rc, rs = R.dgrad(*DEC2, z["kw"], None, z["g1"], None), R.dgrad(*DEC2, None, z["ks"], None, z["gd"])
    bb, bc, bs = (R.bounds(64, r["abs_x0"], r["abs_x1"]) for r in (tb, rc, rs))
    for k in ("x0", "x1"):
        for part, r, b, label in ((vc, rc, bc, "g1 alone"), (vs, rs, bs, "gd alone")):
            err = np.abs(part[k] - r[f"d_{k}"])
            print(f"{label}: d_{k}: {float((err / (b[k] + R.ulp32(r[f'd_{k}']))).max()):.4f} of its bound")
            assert np.all(err <= b[k] + R.ulp32(r[f"d_{k}"])), (label, k)
        diff = np.abs(vc[k] + vs[k] - vb[k])
        assert np.all(diff <= bb[k] + bc[k] + bs[k] + R.ulp32(vb[k])), k
        assert np.abs(vc[k]).max() > 0 and np.abs(vs[k]).max() > 0


def test_nothing_leaks_across_the_batch():
    z = R.inputs((2, 3, 5, 7), *DEC2)
    both = run(DEC2, z)
    g1, gd = z["g1"].copy(), z["gd"].copy()
    g1[1] = 0
    gd[1] = 0
    got = run(DEC2, z, arrays=(g1, gd))
    for k in ("x0", "x1"):
        assert not got[k][1].any() and got[k][0].tobytes() == both[k][0].tobytes(), k
        assert both[k][1].any()


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 3, 70), (1, 2, 4, 65)], ids=ids)
def test_outputs_do_not_depend_on_each_other_or_on_the_run(shape):
    z = R.inputs(shape, *DEC2)
    both, again = run(DEC2, z), run(DEC2, z)
    assert both["x0"].tobytes() == again["x0"].tobytes() and both["x1"].tobytes() == again["x1"].tobytes()
    a, b = run(DEC2, z, want=("x0",)), run(DEC2, z, want=("x1",))
    assert a["x0"].tobytes() == both["x0"].tobytes() and b["x1"].tobytes() == both["x1"].tobytes()
    moved = run(DEC2, z, shifted=True)
    assert moved["x0"].tobytes() == both["x0"].tobytes() and moved["x1"].tobytes() == both["x1"].tobytes()


def test_capped_grids_walk_many_tiles_with_the_bytes_of_any_grid():
    B, L, H, W = BIG
    assert B * L * ((H + 1) // 2) * ((W + 63) // 64) == 60       # tiles: capped workgroups walk many
    z, t = R.inputs(BIG, *DEC2), R.truth(BIG, *DEC2)
    own = run(DEC2, z)
    check(own, DEC2, t, f"128+64->64 {ids(BIG)}")
    for n in (1, 3, 7):
        other = run(DEC2, z, max_workgroups=n)
        assert other["x0"].tobytes() == own["x0"].tobytes() and other["x1"].tobytes() == own["x1"].tobytes(), n
    alone0, alone1 = run(DEC2, z, want=("x0",), max_workgroups=3), run(DEC2, z, want=("x1",), max_workgroups=7)
    for other in (alone0, alone1):
        assert all(other[k].tobytes() == own[k].tobytes() for k in other)


def test_default_pitch_and_python_checks_on_the_device():
    shape = (1, 2, 3, 70)
    z, t = R.inputs(shape, *DEC2), R.truth(shape, *DEC2)
    f = dec2_block.convupn_dgrad
    w, s, g1, gd = torch.from_numpy(z["kw"].copy()).cuda(), torch.from_numpy(z["ks"].copy()).cuda(), device(z["g1"]), device(z["gd"])
    g = f(w, s.view(64, 192, 1, 1, 1), g1, gd)
    assert tuple(g["x0"].shape) == (1, 2, 8, 2, 35, 16) and g["x0"].lw == 35
    assert tuple(g["x1"].shape) == (1, 2, 4, 3, 73, 16) and g["x1"].lw == 70
    check({k: v.cpu().numpy() for k, v in g.items()}, DEC2, t, "default pitch0")
    with pytest.raises(ValueError, match="overlaps"):
        f(w, s, g1, gd, want=("x1",), out={"x1": gd})
    with pytest.raises(ValueError, match="must match"):
        f(w, s, g1, device(z["gd"][:, :, :1]))
    with pytest.raises(ValueError, match="must match"):
        f(w, s, g1, gd, want=("x1",), out={"x1": torch.empty_like(g1)[:, :1].contiguous()})
    with pytest.raises(ValueError, match="pitch0"):
        f(w, s, g1, gd, want=("x0",), out={"x0": torch.empty(1, 2, 8, 2, 34, 16, device="cuda")})
    with pytest.raises(ValueError, match="does not split"):            # a four-plane x0 says c0 = 64: 192 is not 64 + 128
        f(w, s, g1, gd, want=("x0",), out={"x0": torch.empty(1, 2, 4, 2, 35, 16, device="cuda")})
    with pytest.raises(ValueError, match="out holds"):
        f(w, s, g1, gd, want=("x1",), out={"x0": torch.empty(1, 2, 8, 2, 35, 16, device="cuda")})
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(R.to_c16(z["g1"]), 1)
        bad.lw = 70
        f(w, None, bad, None)
    with pytest.raises(ValueError, match=r"\[64, 192, 3, 3, 3\]"):
        f(w.view(64, 192, 27), s, g1, gd)
    with pytest.raises(ValueError, match=r"\[64, 192\]"):               # the two weights disagree
        f(w, s[:, :160].contiguous(), g1, gd)
    with pytest.raises(ValueError, match=r"\[64, 96, 3, 3, 3\] or \[64, 128, 3, 3, 3\]"):     # no sum the entry takes
        f(torch.zeros(64, 100, 3, 3, 3, device="cuda"), s, g1, gd)
    with pytest.raises(ValueError, match="contiguous"):
        f(w, s.t().contiguous().t(), g1, gd)
    with pytest.raises(ValueError, match="both None"):
        f(w, s, None, None)
    with pytest.raises(ValueError, match="needs weight"):
        f(None, s, g1, gd)
    # 128 input channels: 64 + 64 has to be said, through c0 or through out['x0']
    tr = (64, 64, 64)
    z2, t2 = R.inputs((2, 3, 5, 7), *tr), R.truth((2, 3, 5, 7), *tr)
    w2, s2, a1, ad = torch.from_numpy(z2["kw"].copy()).cuda(), torch.from_numpy(z2["ks"].copy()).cuda(), device(z2["g1"]), device(z2["gd"])
    with pytest.raises(ValueError, match=r"64 \+ 64 or as 128 \+ 0"):
        f(w2, s2, a1, ad)
    with pytest.raises(ValueError, match="does not split"):
        f(w2, s2, a1, ad, c0=128)
    said = f(w2, s2, a1, ad, c0=64)
    assert tuple(said["x0"].shape) == (2, 3, 4, 3, 4, 16) and tuple(said["x1"].shape) == (2, 3, 4, 5, 10, 16)
    check({k: v.cpu().numpy() for k, v in said.items()}, tr, t2, "c0=64")
    shown = f(w2, s2, a1, ad, out={"x0": torch.empty(2, 3, 4, 3, 4, 16, device="cuda")})
    assert all(torch.equal(shown[k], said[k]) for k in said)
