"""The input-gradient kernel of the last decoder convolution (v2ce_conv32_dgrad through last_conv.conv32_dgrad) on the GPU
against torch's f64 conv3d input gradient (tests/golden/.lastconv_dgrad/) and the numpy restatement
(tests/last_conv_dgrad_ref.py).

Bound (from the header's precision contract, not from what the kernel gives):
  d_x    |err| <= (V2CE_DGRAD_TERMS + 1) 2^-24 abs_terms + V2CE_DGRAD_TERMS 2^-126: an f32 sum of V2CE_DGRAD_TERMS exact
         products in some fixed order (abs_terms = the f64 sum of |terms| of the element), and what is flushed below the
         normal range;
  d_res  a copy: the bytes of where(y > 0, upstream, 0).
Every result is printed as a fraction of its bound, next to the deviation of torch's own f32 run (ref32_dev)."""
import functools

import numpy as np
import pytest
import torch

from tests import last_conv_dgrad_ref as D
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import hip, last_conv

pytestmark = pytest.mark.gpu

SMALL = [n for n in sorted(CASES) if n not in KERNEL_ONLY]


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
    """[B, 32, L, H, W] -> the kernel's channels-last-16 tensor at the activation pitch, padding columns NaN; shifted: the
    base pointer 16 bytes past a 256-byte boundary."""
    W = a.shape[-1]
    t = offset_copy(D.to_c16(a, D.pitch_of(W)), 4 if shifted else 0)
    t.lw, t.c16 = W, True
    return t


def run(z, masked=True, shifted=False, upstream=None, weight=None, **kw):
    """-> {name: the whole channels-last-16 output as numpy, padding columns included}."""
    up = z["upstream"] if upstream is None else upstream
    w = torch.from_numpy(z["weight"] if weight is None else weight).cuda()
    y = device(z["y"], shifted) if masked else None
    g = last_conv.conv32_dgrad(w, y, device(up, shifted), **kw)
    torch.cuda.synchronize()
    for t in g.values():
        assert t.lw == up.shape[-1] and t.c16
    return {k: v.cpu().numpy() for k, v in g.items()}


def mask_of(z, masked=True, upstream=None):
    up = z["upstream"] if upstream is None else upstream
    return np.where(z["y"] > 0, up, np.float32(0)) if masked else up


def check(got, z, label, sfx="", upstream=None):
    W = z["upstream"].shape[-1]
    for k, a in got.items():
        assert a.shape == D.to_c16(z["upstream"], D.pitch_of(W)).shape and not np.isnan(a).any(), (label, k)  # the NaN padding was not read
        assert not a[:, :, :, :, W:, :].any(), (label, k)          # the outputs' padding columns are exactly zero
    if "x" in got:
        truth, terms = z[f"ref64_dx{sfx}"], z[f"abs_terms_dx{sfx}"]
        err = np.abs(D.from_c16(got["x"], W).astype(np.float64) - truth)
        bound = D.dgrad_bound(terms, hip.DGRAD_TERMS)
        print(f"{label}: d_x: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 "
              f"{float(z[f'ref32_dev_dx{sfx}']):.3e}")
        assert np.all(err <= bound), (label, float(err.max()))
    if "res" in got:
        assert D.from_c16(got["res"], W).tobytes() == mask_of(z, not sfx, upstream).tobytes(), label


@pytest.mark.parametrize("name", SMALL)
def test_kernel_matches_the_f64_truth(name):
    z = case(name)
    got = run(z)
    check(got, z, name)
    if name == "inactive":
        assert not got["x"].any() and not got["res"].any()
    if name == "b1_l2_3x70":
        assert D.pitch_of(70) == 96
    if name == "b1_l1_1x1":                          # the single position sees the centre tap alone
        m = mask_of(z).astype(np.float64).reshape(32)
        centre = z["weight"].astype(np.float64)[:, :, 1, 1, 1]
        want, terms = m @ centre, np.abs(m) @ np.abs(centre)
        err = np.abs(D.from_c16(got["x"], 1).reshape(32).astype(np.float64) - want)
        assert np.all(err <= 33 * 2.0 ** -24 * terms + 32 * 2.0 ** -126)     # 32 terms: the other 26 taps add exact zeros


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_plain_mode_without_y(name):
    z = case(name)
    check(run(z, masked=False), z, name + " plain", "_plain")


def test_nothing_leaks_across_the_batch():
    z = case("b2_l3_5x7")
    both = run(z)
    up = z["upstream"].copy()
    up[1] = 0
    got = run(z, upstream=up)
    assert not got["x"][1].any() and not got["res"][1].any()
    assert got["x"][0].tobytes() == both["x"][0].tobytes() and got["res"][0].tobytes() == both["res"][0].tobytes()


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_outputs_do_not_depend_on_each_other_or_on_the_run(name):
    z = case(name)
    both, again = run(z), run(z)
    assert both["x"].tobytes() == again["x"].tobytes() and both["res"].tobytes() == again["res"].tobytes()
    x, r = run(z, want=("x",)), run(z, want=("res",))
    assert set(x) == {"x"} and set(r) == {"res"}
    check(r, z, name + " res alone")
    assert x["x"].tobytes() == both["x"].tobytes() and r["res"].tobytes() == both["res"].tobytes()
    moved = run(z, shifted=True)
    assert moved["x"].tobytes() == both["x"].tobytes() and moved["res"].tobytes() == both["res"].tobytes()


def test_one_workgroup_walks_every_tile_with_the_bytes_of_any_grid():
    name = KERNEL_ONLY[0]
    z = case(name)
    B, L, H, W = CASES[name]
    assert B * L * ((H + 1) // 2) * ((W + 63) // 64) == 60       # tiles: more than one per workgroup at 1 and 7
    own = run(z)
    check(own, z, name)
    for n in (1, 7):
        other = run(z, max_workgroups=n)
        assert other["x"].tobytes() == own["x"].tobytes() and other["res"].tobytes() == own["res"].tobytes(), n
    again, moved = run(z, max_workgroups=1), run(z, shifted=True)
    for other in (again, moved):
        assert other["x"].tobytes() == own["x"].tobytes() and other["res"].tobytes() == own["res"].tobytes()
    # f32 sums of this case's terms do round (torch's own f32 run is off): the bound is exercised, not met by exact sums
    assert float(z["ref32_dev_dx"]) > 0


def test_out_tensors_and_python_checks_on_the_device():
    z = case("b2_l3_5x7")
    w, y, up = torch.from_numpy(z["weight"]).cuda(), device(z["y"]), device(z["upstream"])
    dx, dr = torch.full_like(up, float("nan")), torch.full_like(up, float("nan"))
    g = last_conv.conv32_dgrad(w, y, up, out={"x": dx, "res": dr})
    assert g["x"] is dx and g["res"] is dr and dx.lw == 7
    check({"x": dx.cpu().numpy(), "res": dr.cpu().numpy()}, z, "out=")
    with pytest.raises(ValueError, match="overlaps"):
        last_conv.conv32_dgrad(w, y, up, want=("res",), out={"res": up})
    with pytest.raises(ValueError, match="overlaps"):
        last_conv.conv32_dgrad(w, y, up, out={"x": dx, "res": dx})
    with pytest.raises(ValueError, match="must match"):
        last_conv.conv32_dgrad(w, device(z["y"][:, :, :2]), up)
    with pytest.raises(ValueError, match="must match"):
        last_conv.conv32_dgrad(w, y, up, want=("x",), out={"x": torch.empty_like(up)[:, :2].contiguous()})
    with pytest.raises(ValueError, match="out holds"):
        last_conv.conv32_dgrad(w, y, up, want=("res",), out={"x": dx})
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(D.to_c16(z["upstream"]), 1)
        bad.lw = z["upstream"].shape[-1]
        last_conv.conv32_dgrad(w, None, bad)
    with pytest.raises(ValueError, match="16-byte"):
        last_conv.conv32_dgrad(w, y, up, want=("x",), out={"x": offset_copy(np.zeros(tuple(up.shape), np.float32), 1)})
    with pytest.raises(ValueError, match=r"\[32, 32, 3, 3, 3\]"):
        last_conv.conv32_dgrad(w.view(32, 32, 27), y, up)
    with pytest.raises(ValueError, match="contiguous"):
        last_conv.conv32_dgrad(w.transpose(0, 1), y, up)
