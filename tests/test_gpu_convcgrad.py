"""v2ce_convc_wgrad and v2ce_convc_dgrad (include/v2ce_hip_convcgrad.h) through their checked Python entries
(conv_grads.convc_wgrad / convc_dgrad) against f64 truths computed on the device from seeded inputs (tests/convc_ref.py,
tests/convn_ref.py; tests/test_convc_grad_cpu.py and tests/test_convn_grad_cpu.py hold the truths to a numpy restatement).

Channel pairs (cin, cout).  convc_ref.PAIRS = (128, 128), (128, 64), (64, 128), (32, 128) run the six shapes of
convn_ref.SMALL ([1,3,20,70] with max_workgroups = the pair count: one share of 60 tiles, a flush of the f32 chain mid-walk
and a partial chain behind it); (128, 128) also runs the walk shape [2,3,43,131] (396 tiles, uneven shares) at the default
grid and at max_workgroups = 97.  convc_ref.WIDE = (256, 256), (512, 512), (512, 32), (32, 512) run [2,3,5,7], [1,2,3,70]
and [1,3,20,70] (one share).  The asymmetric pairs catch a transposed or truncated group index, 512 anything sized for four
groups.  convc_ref.LONG_WALKS: (256, 256) on the walk shape at the default grid (64 pairs, 4 shares of 99 tiles: three flushes
of the f32 chain and three tiles more) and at max_workgroups = 97 (one share), (512, 512) at the default grid (256 pairs, one
share of 396 tiles, twelve flushes, the largest workspace).

Check A, exact.  Integers 1 .. 3 in every value tensor, a normal y with signed zeros for the mask, outputs pre-filled with
NaN.  Every sum is an integer below 2^24, so every element must equal the f64 truth bit for bit; the padding columns of d_x
and d_res are zeros; d_x and d_res have the same bytes at another grid and on buffers moved by 16 bytes; d_weight and
d_shift have the same bytes from run to run.

Check B, contract.  Standard normals; d_weight and d_x inside the header's bounds (the worst element printed as a fraction
of its bound), d_shift within one f32 ulp, d_res a copy.

Then: at (32, 32), (64, 64), (64, 32), (32, 64) the bytes of convn_wgrad / convn_dgrad on [1,3,20,70] and the walk shape at
the default grid, at one share and at max_workgroups = 97; y = None, each output alone, and the refusals of the checked
entries."""
import functools

import numpy as np
import pytest
import torch

from tests import convc_ref as R
from tests import grad_walk_ref as G
from tests import last_conv_ref as CR
from v2ce_toolbox_amd import conv_grads, hip

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = {True: 505, False: 606}
RUNS = R.runs()
IDS = [R.run_id(r) for r in RUNS]
KEYS = {"weight": "d_weight", "shift": "d_shift", "x": "d_x", "res": "d_res"}


@functools.lru_cache(maxsize=4)
def inputs(shape, cin, cout, exact):
    z = {k: v.to(DEV) for k, v in R.inputs(shape, cin, cout, exact, SEEDS[exact]).items()}
    for k in ("x", "y", "upstream"):
        z["c16_" + k] = G.to_c16(z[k], G.pitch_of(shape[3]))
    return z


@functools.lru_cache(maxsize=4)
def truth(shape, cin, cout, exact, with_y=True):
    z = inputs(shape, cin, cout, exact)
    y = z["y"] if with_y else None
    t = dict(R.wgrad_truth(z["x"], y, z["upstream"]))
    t.update(R.dgrad_truth(z["weight"], y, z["upstream"]))
    return t


def nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def run(shape, cin, cout, exact, cap=0, with_y=True, shift=False, wgrad=None, dgrad=None):
    """-> weight, shift, x, res of one call of each entry (convc_* unless given), outputs pre-filled with NaN.  shift: every
    channels-last-16 buffer of the input gradient 16 bytes further inside a larger allocation."""
    wgrad, dgrad = wgrad or conv_grads.convc_wgrad, dgrad or conv_grads.convc_dgrad
    z = inputs(shape, cin, cout, exact)
    B, L, H, W = shape
    pitch = G.pitch_of(W)
    y, up = (z["c16_y"] if with_y else None), z["c16_upstream"]
    g = wgrad(z["c16_x"], y, up, out={"weight": nan((cout, cin, 3, 3, 3)), "shift": nan((cout,))}, max_workgroups=cap)
    sx, sr = (B, L, cin // 16, H, pitch, 16), (B, L, cout // 16, H, pitch, 16)

    def buf(shp, src=None):
        n = int(np.prod(shp))
        if not shift:
            t = nan(shp) if src is None else src
        else:
            t = nan((n + 4,))[4:].view(shp)
            if src is not None:
                t.copy_(src)
        t.lw, t.c16 = W, True
        return t
    y2, up2 = (None if y is None else buf(sr, y)), buf(sr, up)
    assert not shift or up2.data_ptr() % 256 == 16
    g.update(dgrad(z["weight"], y2, up2, out={"x": buf(sx), "res": buf(sr)}, max_workgroups=cap))
    torch.cuda.synchronize()
    assert set(g) == {"weight", "shift", "x", "res"}
    return g


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def mismatch(got, want):
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
    spread = {d: sorted(set(bad[:, d].tolist()))[:12] for d in range(bad.shape[1])}
    return f"{bad.shape[0]} of {got.numel()} elements differ; first (index, got, want): {first}; indices per dim: {spread}"


@pytest.mark.parametrize("run_", RUNS, ids=IDS)
def test_integers_are_bit_exact(run_):
    cin, cout, shape, mult = run_
    cap, W = R.cap_of(cin, cout, mult), shape[3]
    t = truth(shape, cin, cout, True)
    own = run(shape, cin, cout, True, cap)
    for name, key in KEYS.items():
        want = t[key].to(torch.float32)
        assert torch.equal(want.to(torch.float64), t[key]) and float(t[key].max()) < 2 ** 24 and float(t[key].max()) > 0
        got = G.from_c16(own[name], W) if own[name].dim() == 6 else own[name]
        assert got.shape == want.shape, (name, tuple(got.shape))
        assert not torch.isnan(got).any(), (name, "NaN: an element was not written, or a padding column was read")
        assert same_bytes(got, want), (cin, cout, shape, name, mismatch(got, want))
        if own[name].dim() == 6 and own[name].shape[4] > W:
            assert not own[name][:, :, :, :, W:, :].any(), (name, "padding columns must be zeros")
    # the input gradient: the same bytes at another grid and on buffers moved by 16 bytes; the weight gradient: run to run
    other = run(shape, cin, cout, True, 3 if cap != 3 else 5, shift=True)
    again = run(shape, cin, cout, True, cap)
    for name in ("x", "res"):
        assert same_bytes(own[name], other[name]), (cin, cout, shape, name, "grid / base", mismatch(own[name], other[name]))
    for name in KEYS:
        assert same_bytes(own[name], again[name]), (cin, cout, shape, name, "run to run")


def report(label, name, err, bound):
    frac = float((err / bound).max())
    print(f"{label}: {name}: max error {float(err.max()):.3e}, {frac:.3g} of its bound")
    assert np.all(err <= bound), (label, name, float(err.max()), frac)


@pytest.mark.parametrize("run_", RUNS, ids=IDS)
def test_normals_are_inside_the_header_bounds(run_):
    cin, cout, shape, mult = run_
    cap, W = R.cap_of(cin, cout, mult), shape[3]
    t = {k: v.cpu().numpy() for k, v in truth(shape, cin, cout, False).items()}
    own = run(shape, cin, cout, False, cap)
    got = {n: (G.from_c16(v, W) if v.dim() == 6 else v).cpu().numpy() for n, v in own.items()}
    assert not any(np.isnan(v).any() for v in got.values())
    label = f"convc {cin}->{cout} {list(shape)} cap {cap}"
    err = lambda name: np.abs(got[name].astype(np.float64) - t[KEYS[name]])
    report(label, "d_weight", err("weight"), R.wgrad_bound(t["d_weight"], t["abs_weight"], int(np.prod(shape)), hip.WGRAD_CHAIN))
    report(label, "d_shift", np.abs(got["shift"].astype(np.float64) - t["d_shift"].astype(np.float32).astype(np.float64)),
           CR.ulp32(t["d_shift"]))
    report(label, "d_x", err("x"), R.dgrad_bound(t["abs_x"], cout))
    assert np.array_equal(got["res"].view(np.int32), t["d_res"].astype(np.float32).view(np.int32))          # a copy
    for name in ("x", "res"):
        assert not own[name][:, :, :, :, W:, :].any(), name


@pytest.mark.parametrize("shape", R.NARROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin,cout", R.NARROW)
def test_up_to_64_channels_gives_the_bytes_of_the_older_entries(cin, cout, shape):
    """v2ce_convn_* are instances of the widened code with their channel set kept: standard normals, so that an order of
    summation that differed would show."""
    for cap in (0, R.pairs_of(cin, cout), R.PRIME_GRID):
        new = run(shape, cin, cout, False, cap)
        old = run(shape, cin, cout, False, cap, wgrad=conv_grads.convn_wgrad, dgrad=conv_grads.convn_dgrad)
        for name in KEYS:
            assert same_bytes(new[name], old[name]), (cin, cout, shape, cap, name, mismatch(new[name], old[name]))
    if (cin, cout) == (32, 32):                                         # hence the bytes of the 32-channel entries
        new = run(shape, 32, 32, False)
        old = run(shape, 32, 32, False, wgrad=conv_grads.conv32_wgrad, dgrad=conv_grads.conv32_dgrad)
        for name in KEYS:
            assert same_bytes(new[name], old[name]), (shape, name, mismatch(new[name], old[name]))


@pytest.mark.parametrize("cin,cout", ((128, 128), (256, 32)))
def test_without_y_and_each_output_alone(cin, cout):
    shape = (2, 3, 5, 7)
    t = truth(shape, cin, cout, True, with_y=False)
    plain = run(shape, cin, cout, True, with_y=False)
    for name, key in KEYS.items():
        got = G.from_c16(plain[name], shape[3]) if plain[name].dim() == 6 else plain[name]
        assert same_bytes(got, t[key].to(torch.float32)), (name, mismatch(got, t[key].to(torch.float32)))
    assert not same_bytes(plain["weight"], run(shape, cin, cout, True)["weight"])          # the mask does something
    both = run(shape, cin, cout, False)
    z = inputs(shape, cin, cout, False)
    for name in ("weight", "shift"):
        alone = conv_grads.convc_wgrad(z["c16_x"], z["c16_y"], z["c16_upstream"], want=(name,))
        assert set(alone) == {name} and same_bytes(alone[name], both[name]), name
    for name in ("x", "res"):
        alone = conv_grads.convc_dgrad(z["weight"], z["c16_y"], z["c16_upstream"], want=(name,))
        assert set(alone) == {name} and same_bytes(alone[name], both[name]), name
        assert alone[name].lw == shape[3] and alone[name].c16


def test_the_checked_entries_refuse_what_the_header_refuses():
    shape = (1, 2, 3, 70)
    z = inputs(shape, 128, 128, False)
    x, y, up, w = z["c16_x"], z["c16_y"], z["c16_upstream"], z["weight"]
    wg, dg = conv_grads.convc_wgrad, conv_grads.convc_dgrad
    with pytest.raises(ValueError, match="want"):
        wg(x, y, up, want=())
    with pytest.raises(ValueError, match="want"):
        dg(w, y, up, want=("x", "x"))
    with pytest.raises(ValueError, match="max_workgroups"):
        wg(x, y, up, max_workgroups=-1)
    with pytest.raises(ValueError, match="max_workgroups"):
        dg(w, y, up, max_workgroups=-1)
    with pytest.raises(hip.V2ceHipError, match="HIP device"):
        wg(x.cpu(), y, up)
    with pytest.raises(ValueError, match="float32"):
        dg(w, y, up.double())
    for planes in (3, 6):                                               # 48 and 96 channels
        odd = torch.zeros((1, 2, planes, 3, 96, 16), device=DEV)
        with pytest.raises(ValueError, match="channels-last-16"):
            wg(odd, None, up)
        with pytest.raises(ValueError, match="channels-last-16"):
            dg(w, None, odd)
    half = {k: v.to(DEV) for k, v in R.inputs(shape, 128, 64, False, 1).items()}
    half_y, half_up = (G.to_c16(half[k], 96) for k in ("y", "upstream"))
    with pytest.raises(ValueError, match="must match"):
        wg(x, half_y, up)                                               # y with other planes than upstream
    with pytest.raises(ValueError, match="weight must be"):
        dg(half["weight"], y, up)                                       # [64, 128, ...] against 128 channels of upstream
    with pytest.raises(ValueError, match="weight must be"):
        dg(w[:, :96].contiguous(), y, up)
    other = G.to_c16(z["x"][:, :, :, :, :69].contiguous(), 96)
    with pytest.raises(ValueError, match="must match"):
        wg(other, y, up)                                                # another .lw
    with pytest.raises(ValueError, match="16-byte"):
        t = torch.zeros(up.numel() + 1, device=DEV)[1:].view(up.shape)
        t.lw = 70
        dg(w, None, t)
    with pytest.raises(ValueError, match="out holds"):
        wg(x, y, up, want=("weight",), out={"shift": torch.zeros(128, device=DEV)})
    with pytest.raises(ValueError, match="elements"):
        wg(x, y, up, out={"weight": torch.zeros((64, 128, 3, 3, 3), device=DEV)})
    with pytest.raises(ValueError, match="must be"):
        dg(half["weight"], half_y, half_up, out={"x": torch.zeros_like(half_up)})       # 4 planes for cin 128
    with pytest.raises(ValueError, match="overlaps"):
        dg(w, y, up, out={"res": up})
    # the older entries keep their channel set
    with pytest.raises(ValueError, match="channels-last-16"):
        conv_grads.convn_wgrad(x, y, up)
    with pytest.raises(ValueError, match="channels-last-16"):
        conv_grads.convn_dgrad(w, y, up)
    torch.cuda.synchronize()
