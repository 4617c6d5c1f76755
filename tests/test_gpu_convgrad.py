"""The weight-gradient kernel of the last decoder convolution (v2ce_conv32_wgrad through last_conv.conv32_wgrad) on the GPU
against torch's f64 conv3d weight gradient (tests/golden/.lastconv/) and the numpy restatement (tests/last_conv_ref.py).

Bounds (from the header's precision contract, not from what the kernel gives):
  d_weight  |err| <= ulp32(truth) + V2CE_WGRAD_CHAIN 2^-24 abs_terms + N 2^-52 abs_terms: one rounding at the store, an f32
            fmaf chain of at most V2CE_WGRAD_CHAIN positions, N f64 additions above it (N = the number of positions,
            abs_terms = the f64 sum of |terms| of the element);
  d_shift   f64 throughout: within 1 f32 ulp of the truth.
Every result is printed as a fraction of its bound, next to the deviation of torch's own f32 run (ref32_dev)."""
import functools

import numpy as np
import pytest
import torch

from tests import last_conv_ref as R
from tests.make_last_conv_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import hip, last_conv

pytestmark = pytest.mark.gpu

SMALL = [n for n in sorted(CASES) if n not in KERNEL_ONLY]


@functools.lru_cache(maxsize=None)
def case(name):
    return R.load_case(name)


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
    t = offset_copy(R.to_c16(a, R.pitch_of(W)), 4 if shifted else 0)
    t.lw, t.c16 = W, True
    return t


def run(z, masked=True, shifted=False, **kw):
    x, y, up = device(z["t"], shifted), device(z["y"], shifted) if masked else None, device(z["upstream"], shifted)
    g = last_conv.conv32_wgrad(x, y, up, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def check(got, z, label, sfx=""):
    n = z["t"].size // 32
    if "weight" in got:
        truth, terms = z[f"ref64_dM{sfx}"], z[f"abs_terms_dM{sfx}"]
        err = np.abs(got["weight"].astype(np.float64) - truth)
        bound = R.wgrad_bound(truth, terms, n, hip.WGRAD_CHAIN)
        print(f"{label}: d_weight: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 "
              f"{float(z[f'ref32_dev_dM{sfx}']):.3e}")
        assert got["weight"].shape == (32, 32, 3, 3, 3) and np.all(err <= bound), (label, float(err.max()))
    if "shift" in got:
        truth = z[f"ref64_d_shift{sfx}"]
        err = np.abs(got["shift"].astype(np.float64) - truth.astype(np.float32).astype(np.float64))
        bound = R.ulp32(truth)
        print(f"{label}: d_shift: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 "
              f"{float(z[f'ref32_dev_d_shift{sfx}']):.3e}")
        assert np.all(err <= bound), (label, float(err.max()))


@pytest.mark.parametrize("name", SMALL)
def test_kernel_matches_the_f64_truth(name):
    z = case(name)
    got = run(z)
    check(got, z, name)
    assert not np.isnan(got["weight"]).any() and not np.isnan(got["shift"]).any()      # the NaN padding was not read
    if name == "inactive":
        assert not got["weight"].any() and not got["shift"].any()
    if name == "b1_l2_3x70":
        assert R.pitch_of(70) == 96


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_plain_mode_without_y(name):
    z = case(name)
    check(run(z, masked=False), z, name + " plain", "_plain")


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_outputs_do_not_depend_on_each_other_or_on_the_run(name):
    z = case(name)
    both, again = run(z), run(z)
    assert both["weight"].tobytes() == again["weight"].tobytes() and both["shift"].tobytes() == again["shift"].tobytes()
    w, s = run(z, want=("weight",)), run(z, want=("shift",))
    assert set(w) == {"weight"} and set(s) == {"shift"}
    assert w["weight"].tobytes() == both["weight"].tobytes() and s["shift"].tobytes() == both["shift"].tobytes()
    moved = run(z, shifted=True)
    assert moved["weight"].tobytes() == both["weight"].tobytes() and moved["shift"].tobytes() == both["shift"].tobytes()


def test_one_workgroup_walks_every_tile_and_flushes_its_chain():
    name = KERNEL_ONLY[0]
    z = case(name)
    B, L, H, W = CASES[name]
    tiles = B * L * ((H + 1) // 2) * ((W + 63) // 64)
    assert tiles * 128 > hip.WGRAD_CHAIN and B * L * H * W > hip.WGRAD_CHAIN       # at least one flush before the last
    one = run(z, max_workgroups=1)
    check(one, z, name + " max_workgroups=1")
    again = run(z, max_workgroups=1)
    assert one["weight"].tobytes() == again["weight"].tobytes() and one["shift"].tobytes() == again["shift"].tobytes()
    for n in (0, 7):                                  # the grid changes the f64 order only
        other = run(z, max_workgroups=n)
        check(other, z, f"{name} max_workgroups={n}")
    # f32 sums of this case's terms do round (torch's own f32 run is off): the chains are exercised, not bypassed by exact sums
    assert float(z["ref32_dev_dM"]) > 0


def test_out_tensors_and_python_checks_on_the_device():
    z = case("b2_l3_5x7")
    x, y, up = device(z["t"]), device(z["y"]), device(z["upstream"])
    dw, ds = torch.full((32, 32, 3, 3, 3), float("nan"), device="cuda"), torch.full((32,), float("nan"), device="cuda")
    g = last_conv.conv32_wgrad(x, y, up, out={"weight": dw, "shift": ds})
    assert g["weight"] is dw and g["shift"] is ds
    check({"weight": dw.cpu().numpy(), "shift": ds.cpu().numpy()}, z, "out=")
    with pytest.raises(ValueError, match="overlaps"):
        last_conv.conv32_wgrad(x, y, up, want=("shift",), out={"shift": up.view(-1)[:32]})
    with pytest.raises(ValueError, match="must match"):
        last_conv.conv32_wgrad(x, y, device(z["upstream"][:, :, :2]))
    with pytest.raises(ValueError, match="out holds"):
        last_conv.conv32_wgrad(x, y, up, want=("shift",), out={"weight": dw})
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(R.to_c16(z["t"]), 1)
        bad.lw = z["t"].shape[-1]
        last_conv.conv32_wgrad(bad, y, up)
