"""The input-gradient kernel of the last decoder block's conv1 and shortcut (v2ce_convup_dgrad through
last_block.convup_dgrad) on the GPU against torch's f64 conv3d input gradients and upsample backward
(tests/golden/.lastblock_dgrad/) and the numpy restatement (tests/last_block_dgrad_ref.py).

Bound (from the header's precision contract, not from what the kernel gives), plus one ulp of the truth for its rounding:
  d_x1  |err| <= (n + 1) 2^-24 abs_terms + n 2^-126 with n = V2CE_UPDGRAD_TERMS: an f32 sum of n exact products in some
        fixed order (abs_terms = the f64 sum of |terms| of the element), and what is flushed below the normal range;
  d_x0  the same with n = V2CE_UPDGRAD_TERMS times the number of output positions of the source pixel (1, 2 or 4).
Every tensor goes in at pitch = W + 3 and pitch0 = W0 + 5 with NaN in the inputs' padding columns and NaN all over the
outputs.  Every result is printed as a fraction of its bound, next to the deviation of torch's own f32 run (ref32_dev)."""
import functools

import numpy as np
import pytest
import torch

from tests import last_block_dgrad_ref as D
from tests.make_last_block_dgrad_goldens import CASES
from tests.make_last_block_goldens import KERNEL_ONLY
from v2ce_toolbox_amd import hip, last_block

pytestmark = pytest.mark.gpu

BIG = KERNEL_ONLY[0]
SMALL = [n for n in sorted(CASES) if n != BIG]


@functools.lru_cache(maxsize=None)
def case(name):
    return D.load_case(name)


def offset_copy(a, elems):
    """A device copy of `a` whose first element sits `elems` floats past an allocation's start."""
    a = np.ascontiguousarray(a, np.float32)
    flat = torch.zeros(a.size + elems + 64, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 256 == 0
    v = flat[elems:elems + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def device(a, shifted=False):
    """[B, 32, L, H, W] -> the kernel's channels-last-16 tensor at pitch W + 3, padding columns NaN; shifted: the base
    pointer 16 bytes past a 256-byte boundary."""
    W = a.shape[-1]
    t = offset_copy(D.to_c16(a, W + 3), 4 if shifted else 0)
    t.lw, t.c16 = W, True
    return t


def run(z, g1=True, gd=True, shifted=False, want=("x0", "x1"), arrays=None, **kw):
    """-> {name: the whole channels-last-16 output as numpy, padding columns included}."""
    a1, ad = arrays if arrays is not None else (z["g1"], z["gd"])
    B, _, L, H, W = a1.shape
    H0, W0 = (H + 1) // 2, (W + 1) // 2
    shape = {"x0": (B, L, 4, H0, W0 + 5, 16), "x1": (B, L, 2, H, W + 3, 16)}
    out = {n: offset_copy(np.full(shape[n], np.nan, np.float32), 4 if shifted else 0) for n in want}
    w, s = torch.from_numpy(z["kw"]).cuda(), torch.from_numpy(z["ks"]).cuda()
    g = last_block.convup_dgrad(w if g1 else None, s if gd else None, device(a1, shifted) if g1 else None,
                                device(ad, shifted) if gd else None, want=want, out=out, **kw)
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
        B, L, G, H, _, _ = a.shape
        res[k] = np.ascontiguousarray(a[:, :, :, :, :lw, :].transpose(0, 2, 5, 1, 3, 4).reshape(B, G * 16, L, H, lw)).astype(np.float64)
    return res


def bounds(z, abs0=None, abs1=None):
    a0, a1 = (z["abs_terms_d_x0"], z["abs_terms_d_x1"]) if abs0 is None else (abs0, abs1)
    H, W = a1.shape[3], a1.shape[4]
    n0 = hip.UPDGRAD_TERMS * D.pooled(np.ones((1, 1, 1, H, W)))
    return {"x0": D.dgrad_bound(a0, n0), "x1": D.dgrad_bound(a1, hip.UPDGRAD_TERMS)}


def check(got, z, label):
    W = z["ref64_d_x1"].shape[-1]
    vals, b = logical(got, W), bounds(z)
    for k, v in vals.items():
        truth = z[f"ref64_d_{k}"]
        err, bound = np.abs(v - truth), b[k] + D.ulp32(truth)
        print(f"{label}: d_{k}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 "
              f"{float(z[f'ref32_dev_d_{k}']):.3e}")
        assert v.shape == truth.shape and np.all(err <= bound), (label, k, float(err.max()))


@pytest.mark.parametrize("name", SMALL)
def test_kernel_matches_the_f64_truth(name):
    z = case(name)
    got = run(z)
    check(got, z, name)
    if name == "zero":
        assert not got["x0"].any() and not got["x1"].any()
    if name == "b1_l2_4x65":
        # the last tile is one column wide: source column 32 collects output column 64 alone
        v = logical(got, 65)
        dX = D.dgrad(z["kw"], z["ks"], z["g1"], z["gd"])["d_X"]
        want = dX[:, :64, :, 0::2, 64] + dX[:, :64, :, 1::2, 64]
        assert np.all(np.abs(v["x0"][..., 32] - want) <= bounds(z)["x0"][..., 32] + D.ulp32(want))
        assert np.abs(want).max() > 0


def test_shares_add_up():
    """The g1-only call plus the gd-only call is the combined call: each of the three is within its own bound of its exact
    value, and the exact values add up, so the difference is within the sum of the three bounds (plus the f64 rounding of
    the test's own addition, a 2^-52 relative term that an ulp32 covers)."""
    z = case("b2_l3_5x7")
    both, conv, short = run(z), run(z, gd=False), run(z, g1=False)
    vb, vc, vs = (logical(g, 7) for g in (both, conv, short))
    rc, rs = D.dgrad(z["kw"], None, z["g1"], None), D.dgrad(None, z["ks"], None, z["gd"])
    bb, bc, bs = bounds(z), bounds(z, rc["abs_x0"], rc["abs_x1"]), bounds(z, rs["abs_x0"], rs["abs_x1"])
    for k in ("x0", "x1"):
        for part, r, b, label in ((vc, rc, bc, "g1 alone"), (vs, rs, bs, "gd alone")):
            err = np.abs(part[k] - r[f"d_{k}"])
            print(f"{label}: d_{k}: {float((err / (b[k] + D.ulp32(r[f'd_{k}']))).max()):.4f} of its bound")
            assert np.all(err <= b[k] + D.ulp32(r[f"d_{k}"])), (label, k)
        diff = np.abs(vc[k] + vs[k] - vb[k])
        assert np.all(diff <= bb[k] + bc[k] + bs[k] + D.ulp32(vb[k])), k
        assert np.abs(vc[k]).max() > 0 and np.abs(vs[k]).max() > 0


def test_nothing_leaks_across_the_batch():
    z = case("b2_l3_5x7")
    both = run(z)
    g1, gd = z["g1"].copy(), z["gd"].copy()
    g1[1] = 0
    gd[1] = 0
    got = run(z, arrays=(g1, gd))
    for k in ("x0", "x1"):
        assert not got[k][1].any() and got[k][0].tobytes() == both[k][0].tobytes(), k
        assert both[k][1].any()


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70", "b1_l2_4x65"])
def test_outputs_do_not_depend_on_each_other_or_on_the_run(name):
    z = case(name)
    both, again = run(z), run(z)
    assert both["x0"].tobytes() == again["x0"].tobytes() and both["x1"].tobytes() == again["x1"].tobytes()
    a, b = run(z, want=("x0",)), run(z, want=("x1",))
    assert a["x0"].tobytes() == both["x0"].tobytes() and b["x1"].tobytes() == both["x1"].tobytes()
    moved = run(z, shifted=True)
    assert moved["x0"].tobytes() == both["x0"].tobytes() and moved["x1"].tobytes() == both["x1"].tobytes()


def test_capped_grids_walk_many_tiles_with_the_bytes_of_any_grid():
    z = case(BIG)
    B, L, H, W = CASES[BIG]
    assert B * L * ((H + 1) // 2) * ((W + 63) // 64) == 60       # tiles: capped workgroups walk many
    own = run(z)
    check(own, z, BIG)
    for n in (1, 3, 7):
        other = run(z, max_workgroups=n)
        assert other["x0"].tobytes() == own["x0"].tobytes() and other["x1"].tobytes() == own["x1"].tobytes(), n
    again, moved = run(z, max_workgroups=1), run(z, shifted=True)
    alone0, alone1 = run(z, want=("x0",), max_workgroups=3), run(z, want=("x1",), max_workgroups=7)
    for other in (again, moved, alone0, alone1):
        assert all(other[k].tobytes() == own[k].tobytes() for k in other)
    # f32 sums of this case's terms do round (torch's own f32 run is off): the bound is exercised, not met by exact sums
    assert float(z["ref32_dev_d_x1"]) > 0 and float(z["ref32_dev_d_x0"]) > 0


def test_default_pitch_and_python_checks_on_the_device():
    z = case("b1_l2_3x70")
    w, s, g1, gd = torch.from_numpy(z["kw"]).cuda(), torch.from_numpy(z["ks"]).cuda(), device(z["g1"]), device(z["gd"])
    g = last_block.convup_dgrad(w, s.view(32, 96, 1, 1, 1), g1, gd)
    assert tuple(g["x0"].shape) == (1, 2, 4, 2, 35, 16) and g["x0"].lw == 35 and tuple(g["x1"].shape) == tuple(g1.shape)
    check({k: v.cpu().numpy() for k, v in g.items()}, z, "default pitch0")
    with pytest.raises(ValueError, match="overlaps"):
        last_block.convup_dgrad(w, s, g1, gd, want=("x1",), out={"x1": gd})
    with pytest.raises(ValueError, match="must match"):
        last_block.convup_dgrad(w, s, g1, device(z["gd"][:, :, :1]))
    with pytest.raises(ValueError, match="must match"):
        last_block.convup_dgrad(w, s, g1, gd, want=("x1",), out={"x1": torch.empty_like(g1)[:, :1].contiguous()})
    with pytest.raises(ValueError, match="pitch0"):
        last_block.convup_dgrad(w, s, g1, gd, want=("x0",), out={"x0": torch.empty(1, 2, 4, 2, 34, 16, device="cuda")})
    with pytest.raises(ValueError, match="out holds"):
        last_block.convup_dgrad(w, s, g1, gd, want=("x1",), out={"x0": torch.empty(1, 2, 4, 2, 35, 16, device="cuda")})
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(D.to_c16(z["g1"]), 1)
        bad.lw = 70
        last_block.convup_dgrad(w, None, bad, None)
    with pytest.raises(ValueError, match=r"\[32, 96, 3, 3, 3\]"):
        last_block.convup_dgrad(w.view(32, 96, 27), s, g1, gd)
    with pytest.raises(ValueError, match="contiguous"):
        last_block.convup_dgrad(w, s.t().contiguous().t(), g1, gd)
    with pytest.raises(ValueError, match="both None"):
        last_block.convup_dgrad(w, s, None, None)
    with pytest.raises(ValueError, match="needs weight"):
        last_block.convup_dgrad(None, s, g1, gd)
