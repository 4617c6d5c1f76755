"""v2ce_convn_wgrad and v2ce_convn_dgrad (include/v2ce_hip_convngrad.h) through their checked Python entries
(dec2_conv.convn_wgrad / convn_dgrad) against f64 truths computed on the device from seeded inputs (tests/convn_ref.py; the
truths are held to a numpy restatement and to torch.nn.grad by tests/test_convn_grad_cpu.py).

Channel pairs (cin, cout) = (64, 64), (64, 32), (32, 64): the asymmetric ones catch a transposed group index.  Shapes
[B, L, H, W]: the six of convn_ref.SMALL ([1,3,20,70] runs with max_workgroups = the pair count: one share of 60 tiles, a
flush of the f32 chain mid-walk and a partial chain behind it) and the walk shape [2,3,43,131] (396 tiles: the default grids
are at their caps on uneven shares) at the default grid and at max_workgroups = 97.

Check A, exact.  Integers 1 .. 3 in every value tensor, a normal y with signed zeros for the mask, outputs pre-filled with
NaN where the entry takes them.  Every sum is an integer below 2^24, so every element must equal the f64 truth bit for bit;
the padding columns of d_x and d_res are zeros; d_x and d_res have the same bytes at another grid and on buffers moved by
16 bytes; d_weight and d_shift have the same bytes from run to run.

Check B, contract.  Standard normals; d_weight and d_x inside the header's bounds (the worst element printed as a fraction
of its bound), d_shift within one f32 ulp, d_res a copy.

(32, 32): conv32_wgrad / conv32_dgrad and the N-channel entries on the inputs of tests/golden/.lastconv, at the default grid
and at two caps: the bytes recorded from the 32-channel kernels (tests/golden/.gradfold, tests/make_grad_fold_digests.py).
Then y = None, each output alone, and the refusals of the checked entries."""
import functools

import numpy as np
import pytest
import torch

from tests import convn_ref as R
from tests import grad_walk_ref as G
from tests import last_conv_ref as CR
from tests import make_grad_fold_digests as F
from v2ce_toolbox_amd import dec2_conv, hip, last_conv

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = {True: 303, False: 404}
# (shape, max_workgroups as a multiple of the pair count or None: the prime)
RUNS = [(shape, mult) for shape, mult in R.SMALL.items()] + [(R.WALK, 0), (R.WALK, None)]
IDS = ["x".join(map(str, s)) + ("" if m == 0 else "_one_share" if m else "_grid97") for s, m in RUNS]


def cap_of(cin, cout, mult):
    return R.PRIME_GRID if mult is None else mult * R.pairs_of(cin, cout)


@functools.lru_cache(maxsize=None)
def inputs(shape, cin, cout, exact):
    z = {k: v.to(DEV) for k, v in R.inputs(shape, cin, cout, exact, SEEDS[exact]).items()}
    for k in ("x", "y", "upstream"):
        z["c16_" + k] = G.to_c16(z[k], G.pitch_of(shape[3]))
    return z


@functools.lru_cache(maxsize=None)
def truth(shape, cin, cout, exact, with_y=True):
    z = inputs(shape, cin, cout, exact)
    y = z["y"] if with_y else None
    t = dict(R.wgrad_truth(z["x"], y, z["upstream"]))
    t.update(R.dgrad_truth(z["weight"], y, z["upstream"]))
    return t


def nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def run(shape, cin, cout, exact, cap=0, with_y=True, shift=False):
    """-> weight, shift, x, res of one call of each entry, outputs pre-filled with NaN.  shift: every channels-last-16 buffer
    of the input gradient 16 bytes further inside a larger allocation."""
    z = inputs(shape, cin, cout, exact)
    B, L, H, W = shape
    pitch = G.pitch_of(W)
    y, up = (z["c16_y"] if with_y else None), z["c16_upstream"]
    g = dec2_conv.convn_wgrad(z["c16_x"], y, up, out={"weight": nan((cout, cin, 3, 3, 3)), "shift": nan((cout,))},
                              max_workgroups=cap)
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
    g.update(dec2_conv.convn_dgrad(z["weight"], y2, up2, out={"x": buf(sx), "res": buf(sr)}, max_workgroups=cap))
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


KEYS = {"weight": "d_weight", "shift": "d_shift", "x": "d_x", "res": "d_res"}


@pytest.mark.parametrize("run_", RUNS, ids=IDS)
@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_integers_are_bit_exact(cin, cout, run_):
    shape, mult = run_
    cap, W = cap_of(cin, cout, mult), shape[3]
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
@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_normals_are_inside_the_header_bounds(cin, cout, run_):
    shape, mult = run_
    cap, W = cap_of(cin, cout, mult), shape[3]
    t = {k: v.cpu().numpy() for k, v in truth(shape, cin, cout, False).items()}
    own = run(shape, cin, cout, False, cap)
    got = {n: (G.from_c16(v, W) if v.dim() == 6 else v).cpu().numpy() for n, v in own.items()}
    assert not any(np.isnan(v).any() for v in got.values())
    label = f"convn {cin}->{cout} {list(shape)} cap {cap}"
    err = lambda name: np.abs(got[name].astype(np.float64) - t[KEYS[name]])
    report(label, "d_weight", err("weight"), R.wgrad_bound(t["d_weight"], t["abs_weight"], int(np.prod(shape)), hip.WGRAD_CHAIN))
    report(label, "d_shift", np.abs(got["shift"].astype(np.float64) - t["d_shift"].astype(np.float32).astype(np.float64)),
           CR.ulp32(t["d_shift"]))
    report(label, "d_x", err("x"), R.dgrad_bound(t["abs_x"], cout))
    assert np.array_equal(got["res"].view(np.int32), t["d_res"].astype(np.float32).view(np.int32))          # a copy
    for name in ("x", "res"):
        assert not own[name][:, :, :, :, W:, :].any(), name


@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_without_y_and_each_output_alone(cin, cout):
    shape = (2, 3, 5, 7)
    z = inputs(shape, cin, cout, True)
    t = truth(shape, cin, cout, True, with_y=False)
    plain = run(shape, cin, cout, True, with_y=False)
    for name, key in KEYS.items():
        got = G.from_c16(plain[name], shape[3]) if plain[name].dim() == 6 else plain[name]
        assert same_bytes(got, t[key].to(torch.float32)), (name, mismatch(got, t[key].to(torch.float32)))
    assert not same_bytes(plain["weight"], run(shape, cin, cout, True)["weight"])          # the mask does something
    both = run(shape, cin, cout, False)
    z = inputs(shape, cin, cout, False)
    for name in ("weight", "shift"):
        alone = dec2_conv.convn_wgrad(z["c16_x"], z["c16_y"], z["c16_upstream"], want=(name,))
        assert set(alone) == {name} and same_bytes(alone[name], both[name]), name
    for name in ("x", "res"):
        alone = dec2_conv.convn_dgrad(z["weight"], z["c16_y"], z["c16_upstream"], want=(name,))
        assert set(alone) == {name} and same_bytes(alone[name], both[name]), name
        assert alone[name].lw == shape[3] and alone[name].c16


@pytest.mark.parametrize("name", F.CASES)
def test_32_to_32_gives_the_bytes_of_the_32_channel_entries(name):
    """conv32_wgrad / conv32_dgrad forward to the kernels of convn_wgrad / convn_dgrad: both must still give the bytes that
    the 32-channel kernels gave while they were kernels of their own (tests/make_grad_fold_digests.py), for every case, cap
    and output, and so the bytes of each other."""
    want = F.load()
    old = F.conv32_outputs(name, last_conv.conv32_wgrad, last_conv.conv32_dgrad)
    new = F.conv32_outputs(name, dec2_conv.convn_wgrad, dec2_conv.convn_dgrad)
    keys = [k for k in want if k.startswith(f"conv32/{name}/")]
    assert sorted(old) == sorted(new) == sorted(keys) and len(keys) == 4 * len(F.CONV32_CAPS) + 2
    for k in keys:
        assert same_bytes(old[k], new[k]), (k, mismatch(new[k], old[k]))
        assert F.digest(old[k]) == want[k], (k, "conv32 entry: not the bytes of the 32-channel kernel")
        assert F.digest(new[k]) == want[k], (k, "convn entry: not the bytes of the 32-channel kernel")


def test_the_checked_entries_refuse_what_the_header_refuses():
    shape = (1, 2, 3, 70)
    z = inputs(shape, 64, 64, False)
    x, y, up, w = z["c16_x"], z["c16_y"], z["c16_upstream"], z["weight"]
    wg, dg = dec2_conv.convn_wgrad, dec2_conv.convn_dgrad
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
    three = torch.zeros((1, 2, 3, 3, 96, 16), device=DEV)               # 48 channels
    with pytest.raises(ValueError, match="channels-last-16"):
        wg(three, None, up)
    with pytest.raises(ValueError, match="channels-last-16"):
        dg(w, None, three)
    half = inputs(shape, 64, 32, False)
    with pytest.raises(ValueError, match="must match"):
        wg(x, half["c16_y"], up)                                        # y with other planes than upstream
    with pytest.raises(ValueError, match="weight must be"):
        dg(half["weight"], y, up)                                       # [32, 64, ...] against 64 channels of upstream
    with pytest.raises(ValueError, match="weight must be"):
        dg(w[:, :48].contiguous(), y, up)
    other = G.to_c16(z["x"][:, :, :, :, :69].contiguous(), 96)
    with pytest.raises(ValueError, match="must match"):
        wg(other, y, up)                                                # another .lw
    with pytest.raises(ValueError, match="16-byte"):
        t = torch.zeros(up.numel() + 1, device=DEV)[1:].view(up.shape)
        t.lw = 70
        dg(w, None, t)
    with pytest.raises(ValueError, match="out holds"):
        wg(x, y, up, want=("weight",), out={"shift": torch.zeros(64, device=DEV)})
    with pytest.raises(ValueError, match="elements"):
        wg(x, y, up, out={"weight": torch.zeros((32, 64, 3, 3, 3), device=DEV)})
    with pytest.raises(ValueError, match="must be"):
        dg(half["weight"], half["c16_y"], half["c16_upstream"], out={"x": torch.zeros_like(half["c16_upstream"])})   # 2 planes for cin 64
    with pytest.raises(ValueError, match="overlaps"):
        dg(w, y, up, out={"res": up})
    torch.cuda.synchronize()
