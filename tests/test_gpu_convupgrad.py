"""The weight-gradient kernel of the last decoder block's conv1 and shortcut (v2ce_convup_wgrad through
last_block.convup_wgrad) on the GPU against torch's f64 conv3d weight gradient on the materialised upsample + concat
(tests/golden/.lastblock/).

Bounds (from the header's precision contract, not from what the kernel gives):
  d_weight, d_short  |err| <= ulp32(truth) + V2CE_UPWGRAD_CHAIN 2^-24 abs_terms + N 2^-52 abs_terms: one rounding at the
                     store, an f32 fmaf chain of at most V2CE_UPWGRAD_CHAIN positions, N f64 additions above it (N = the
                     number of positions, abs_terms = the f64 sum of |terms| of the element);
  d_short_bias       f64 throughout: within 1 f32 ulp of the truth.
Every result is printed as a fraction of its bound, next to the deviation of torch's own f32 run (ref32_dev)."""
import functools

import numpy as np
import pytest
import torch

from tests import last_block_ref as R
from tests.make_last_block_goldens import CASES, KERNEL_ONLY
from v2ce_toolbox_amd import hip, last_block

pytestmark = pytest.mark.gpu

SMALL = [n for n in sorted(CASES) if n not in KERNEL_ONLY]
KEYS = {"weight": ("ref64_dW", "abs_terms_dW", "ref32_dev_dW"), "short": ("ref64_dMd", "abs_terms_dMd", "ref32_dev_dMd")}


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
    """[B, 32, L, H, W] or the source [B, 64, L, H0, W0] -> the kernel's channels-last-16 tensor at the activation pitch,
    padding columns NaN; shifted: the base pointer 16 bytes past a 256-byte boundary."""
    W = a.shape[-1]
    c = R.src_to_c16(a, R.pitch_of(W)) if a.shape[1] == 64 else R.to_c16(a, R.pitch_of(W))
    t = offset_copy(c, 4 if shifted else 0)
    t.lw, t.c16 = W, True
    return t


def run(z, shifted=False, g1=None, **kw):
    x0, x1, gd = device(z["x0"], shifted), device(z["x1"], shifted), device(z["gd"], shifted)
    g = last_block.convup_wgrad(x0, x1, device(z["g1"] if g1 is None else g1, shifted), gd, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def bounds(z, name):
    truth, terms, _ = (z[k] for k in KEYS[name])
    return R.wgrad_bound(truth, terms, z["x1"].size // 32, hip.UPWGRAD_CHAIN)


def check(got, z, label):
    for name in ("weight", "short"):
        if name in got:
            truth, dev32 = z[KEYS[name][0]], float(z[KEYS[name][2]])
            err = np.abs(got[name].astype(np.float64) - truth)
            bound = bounds(z, name)
            print(f"{label}: d_{name}: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 {dev32:.3e}")
            assert got[name].shape == truth.shape and np.all(err <= bound), (label, name, float(err.max()))
    if "short_bias" in got:
        truth = z["ref64_d_sum"]
        err = np.abs(got["short_bias"].astype(np.float64) - truth.astype(np.float32).astype(np.float64))
        bound = R.ulp32(truth)
        print(f"{label}: d_short_bias: max error {err.max():.3e}, {float((err / bound).max()):.4f} of its bound; torch f32 "
              f"{float(z['ref32_dev_d_sum']):.3e}")
        assert np.all(err <= bound), (label, float(err.max()))


def same(a, b):
    return set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", SMALL)
def test_kernel_matches_the_f64_truth(name):
    z = case(name)
    got = run(z)
    assert set(got) == {"weight", "short", "short_bias"}
    check(got, z, name)
    assert not any(np.isnan(v).any() for v in got.values())      # the NaN padding of neither pitch was read
    if name == "zero":
        assert not any(v.any() for v in got.values())
    if name == "b1_l2_3x70":
        assert R.pitch_of(70) == 96 and R.pitch_of(35) == 35
    if name == "b1_l1_1x1":                                       # only the centre tap sees the single position
        nz = got["weight"].reshape(32, 96, 27).any(axis=(0, 1))
        assert nz.tolist() == [k == 13 for k in range(27)]


def test_source_pitch_padding_is_not_read():
    """A source pitch above W0 (pitch0 = 40 for W0 = 35, NaN behind the row) and the same bytes as at pitch0 = W0."""
    z = case("b1_l2_3x70")
    x1, g1, gd = device(z["x1"]), device(z["g1"]), device(z["gd"])
    wide = torch.from_numpy(R.src_to_c16(z["x0"], 40)).cuda()
    wide.lw = 35
    got = {k: v.cpu().numpy() for k, v in last_block.convup_wgrad(wide, x1, g1, gd).items()}
    check(got, z, "pitch0 = 40")
    assert same(got, run(z))


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_the_centre_tap_is_the_shortcut(name):
    """With g1 := gd the tap (1, 1, 1) of d_weight sums the terms of d_short: both lie within their bounds of the same truth."""
    z = case(name)
    got = run(z, g1=z["gd"])
    centre, short = got["weight"][:, :, 1, 1, 1].astype(np.float64), got["short"].astype(np.float64)
    b = bounds(z, "short")
    frac = np.abs(centre - short) / (2 * b)
    print(f"{name}: |centre tap - d_short| is {float(frac.max()):.4f} of the two bounds")
    assert np.all(np.abs(centre - z["ref64_dMd"]) <= b) and np.all(np.abs(short - z["ref64_dMd"]) <= b)
    assert np.all(np.abs(centre - short) <= 2 * b)


@pytest.mark.parametrize("name", ["b2_l3_5x7", "b1_l2_3x70"])
def test_outputs_do_not_depend_on_each_other_or_on_the_run(name):
    z = case(name)
    both = run(z)
    assert same(both, run(z))
    for want in (("weight",), ("short",), ("short_bias",), ("short", "short_bias"), ("weight", "short_bias")):
        part = run(z, want=want)
        assert set(part) == set(want) and all(part[k].tobytes() == both[k].tobytes() for k in want), want
    assert same(both, run(z, shifted=True))


def test_inputs_an_output_does_not_need_may_be_missing():
    z = case("b2_l3_5x7")
    x0, x1, g1, gd = (device(z[k]) for k in ("x0", "x1", "g1", "gd"))
    both = run(z)
    w = last_block.convup_wgrad(x0, x1, g1, None, want=("weight",))
    s = last_block.convup_wgrad(x0, x1, None, gd, want=("short", "short_bias"))
    assert w["weight"].cpu().numpy().tobytes() == both["weight"].tobytes()
    assert s["short"].cpu().numpy().tobytes() == both["short"].tobytes()
    assert s["short_bias"].cpu().numpy().tobytes() == both["short_bias"].tobytes()


def test_one_share_walks_every_tile_and_flushes_its_chain():
    name = KERNEL_ONLY[0]
    z = case(name)
    B, L, H, W = CASES[name]
    tiles = B * L * ((H + 1) // 2) * ((W + 63) // 64)
    assert tiles * 128 > hip.UPWGRAD_CHAIN and B * L * H * W > hip.UPWGRAD_CHAIN   # at least one flush before the last
    one = run(z, max_workgroups=1)
    check(one, z, name + " max_workgroups=1")
    assert same(one, run(z, max_workgroups=1))
    assert same(one, run(z, max_workgroups=3))         # three workgroups are one share as well
    for n in (0, 7):                                  # the grid changes the f64 order only
        check(run(z, max_workgroups=n), z, f"{name} max_workgroups={n}")
    # f32 sums of this case's terms do round (torch's own f32 run is off): the chains are exercised, not bypassed by exact sums
    assert float(z["ref32_dev_dW"]) > 0 and float(z["ref32_dev_dMd"]) > 0


def test_out_tensors_and_python_checks_on_the_device():
    z = case("b2_l3_5x7")
    x0, x1, g1, gd = (device(z[k]) for k in ("x0", "x1", "g1", "gd"))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    dw, ds, db = nan(32, 96, 3, 3, 3), nan(32, 96), nan(32)
    g = last_block.convup_wgrad(x0, x1, g1, gd, out={"weight": dw, "short": ds, "short_bias": db})
    assert g["weight"] is dw and g["short"] is ds and g["short_bias"] is db
    check({"weight": dw.cpu().numpy(), "short": ds.cpu().numpy(), "short_bias": db.cpu().numpy()}, z, "out=")
    with pytest.raises(ValueError, match="overlaps"):
        last_block.convup_wgrad(x0, x1, g1, gd, want=("short_bias",), out={"short_bias": gd.view(-1)[:32]})
    with pytest.raises(ValueError, match="overlaps"):
        last_block.convup_wgrad(x0, x1, g1, gd, want=("short_bias",), out={"short_bias": x0.view(-1)[:32]})
    with pytest.raises(ValueError, match="must match x1"):
        last_block.convup_wgrad(x0, x1, device(z["g1"][:, :, :2]), gd)
    with pytest.raises(ValueError, match="must match x1"):
        last_block.convup_wgrad(device(z["x0"][:, :, :2]), x1, g1, gd)
    with pytest.raises(ValueError, match="must match x1"):
        last_block.convup_wgrad(device(z["x0"][:, :, :, :2]), x1, g1, gd)           # H0 = 2 for H = 5
    with pytest.raises(ValueError, match="channels-last-16"):
        last_block.convup_wgrad(x1, x1, g1, gd)                                       # two groups where x0 has four
    with pytest.raises(ValueError, match="out holds"):
        last_block.convup_wgrad(x0, x1, g1, gd, want=("short",), out={"weight": dw})
    with pytest.raises(ValueError, match="elements"):
        last_block.convup_wgrad(x0, x1, g1, gd, want=("short",), out={"short": db})
    with pytest.raises(ValueError, match="needs g1"):
        last_block.convup_wgrad(x0, x1, None, gd)
    with pytest.raises(ValueError, match="need gd"):
        last_block.convup_wgrad(x0, x1, g1, None)
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(R.src_to_c16(z["x0"]), 1)
        bad.lw = z["x0"].shape[-1]
        last_block.convup_wgrad(bad, x1, g1, gd)
    with pytest.raises(ValueError, match="16-byte"):
        bad = offset_copy(R.to_c16(z["gd"]), 1)
        bad.lw = z["gd"].shape[-1]
        last_block.convup_wgrad(x0, x1, g1, bad)
