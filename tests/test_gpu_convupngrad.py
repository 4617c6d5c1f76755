"""v2ce_convupn_wgrad (include/v2ce_hip_convupngrad.h) through its checked Python entry (dec2_block.convupn_wgrad) against
f64 truths computed on the device from seeded inputs (tests/convupn_ref.py; the truths are held to a numpy restatement and to
torch.nn.grad on the materialised upsample + concat by tests/test_convupn_grad_cpu.py).

Channel triples (c0, c1, cout) = (128, 64, 64) -- dec2 --, (64, 64, 32) and (128, 32, 64): asymmetric on both axes, so a
transposed or mis-strided group index cannot cancel.  Shapes [B, L, H, W]: the five of convupn_ref.SMALL ([1,3,20,70] runs
with max_workgroups = the pair count: one share of 60 tiles, a flush of the f32 chain mid-walk and a partial chain behind
it) and the walk shape [2,3,43,131] (396 tiles: the default grid is at its cap on uneven shares) at the default grid and at
max_workgroups = 97.

Check A, exact.  Integers 1 .. 3 in every value tensor, outputs pre-filled with NaN, NaN in the padding columns of every
input.  Every sum is an integer below 2^24, so every element of d_weight, d_short and d_short_bias must equal the f64 truth
bit for bit; the same bytes come out run to run, and each output requested alone has the same bytes.

Check B, contract.  Standard normals; d_weight and d_short inside the header's bound (the worst element printed as a
fraction of its bound), d_short_bias within one f32 ulp.

(64, 32, 32): last_block.convup_wgrad and the N-channel entry on the inputs of tests/golden/.lastblock, at the default grid
and at two caps: the bytes recorded from the 96 -> 32 kernel (tests/golden/.gradfold, tests/make_grad_fold_digests.py).
Then the refusals of the checked entry."""
import functools

import numpy as np
import pytest
import torch

from tests import convupn_ref as R
from tests import grad_walk_ref as G
from tests import make_grad_fold_digests as F
from v2ce_toolbox_amd import dec2_block, hip, last_block

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = {True: 505, False: 606}
# (shape, max_workgroups as a multiple of the pair count or None: the prime)
RUNS = [(shape, mult) for shape, mult in R.SMALL.items()] + [(R.WALK, 0), (R.WALK, None)]
IDS = ["x".join(map(str, s)) + ("" if m == 0 else "_one_share" if m else "_grid97") for s, m in RUNS]
KEYS = {"weight": "d_weight", "short": "d_short", "short_bias": "d_short_bias"}


def cap_of(triple, mult):
    return R.PRIME_GRID if mult is None else mult * R.pairs_of(*triple)


@functools.lru_cache(maxsize=None)
def inputs(shape, triple, exact):
    """The seeded inputs on the device and their channels-last-16 forms at the activation pitches, NaN in the padding."""
    z = {k: v.to(DEV) for k, v in R.inputs(shape, *triple, exact, SEEDS[exact]).items()}
    W = shape[3]
    z["c16_x0"] = G.to_c16(z["x0"], G.pitch_of((W + 1) // 2))
    for k in ("x1", "g1", "gd"):
        z["c16_" + k] = G.to_c16(z[k], G.pitch_of(W))
    return z


@functools.lru_cache(maxsize=None)
def truth(shape, triple, exact):
    z = inputs(shape, triple, exact)
    return R.wgrad_truth(z["x0"], z["x1"], z["g1"], z["gd"])


def nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def run(shape, triple, exact, cap=0, want=dec2_block.WANT):
    """-> the outputs of one call, pre-filled with NaN."""
    z = inputs(shape, triple, exact)
    c0, c1, cout = triple
    shapes = {"weight": (cout, c0 + c1, 3, 3, 3), "short": (cout, c0 + c1), "short_bias": (cout,)}
    g = dec2_block.convupn_wgrad(z["c16_x0"], z["c16_x1"], z["c16_g1"] if "weight" in want else None,
                                 z["c16_gd"] if ("short" in want or "short_bias" in want) else None, want=want,
                                 out={n: nan(shapes[n]) for n in want}, max_workgroups=cap)
    torch.cuda.synchronize()
    assert set(g) == set(want) and all(tuple(g[n].shape) == shapes[n] for n in want)
    return g


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def mismatch(got, want):
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
    spread = {d: sorted(set(bad[:, d].tolist()))[:12] for d in range(bad.shape[1])}
    return f"{bad.shape[0]} of {got.numel()} elements differ; first (index, got, want): {first}; indices per dim: {spread}"


@pytest.mark.parametrize("run_", RUNS, ids=IDS)
@pytest.mark.parametrize("triple", R.TRIPLES, ids=lambda t: "_".join(map(str, t)))
def test_integers_are_bit_exact(triple, run_):
    shape, mult = run_
    cap = cap_of(triple, mult)
    t = truth(shape, triple, True)
    own = run(shape, triple, True, cap)
    for name, key in KEYS.items():
        want = t[key].to(torch.float32)
        assert torch.equal(want.to(torch.float64), t[key]) and 0 < float(t[key].max()) < 2 ** 24
        got = own[name]
        assert not torch.isnan(got).any(), (name, "NaN: an element was not written, or a padding column was read")
        assert same_bytes(got, want), (triple, shape, name, mismatch(got, want))
    again = run(shape, triple, True, cap)
    for name in KEYS:
        assert same_bytes(own[name], again[name]), (triple, shape, name, "run to run")
        alone = run(shape, triple, True, cap, want=(name,))
        assert same_bytes(own[name], alone[name]), (triple, shape, name, "requested alone")


def report(label, name, err, bound):
    frac = float((err / bound).max())
    print(f"{label}: {name}: max error {float(err.max()):.3e}, {frac:.3g} of its bound")
    assert np.all(err <= bound), (label, name, float(err.max()), frac)


@pytest.mark.parametrize("run_", RUNS, ids=IDS)
@pytest.mark.parametrize("triple", R.TRIPLES, ids=lambda t: "_".join(map(str, t)))
def test_normals_are_inside_the_header_bound(triple, run_):
    shape, mult = run_
    cap = cap_of(triple, mult)
    t = {k: v.cpu().numpy() for k, v in truth(shape, triple, False).items()}
    got = {n: v.cpu().numpy() for n, v in run(shape, triple, False, cap).items()}
    assert not any(np.isnan(v).any() for v in got.values())
    label = f"convupn {triple} {list(shape)} cap {cap}"
    n_pos = int(np.prod(shape))
    for name, ab in (("weight", "abs_weight"), ("short", "abs_short")):
        err = np.abs(got[name].astype(np.float64) - t[KEYS[name]])
        report(label, KEYS[name], err, R.bound(t[KEYS[name]], t[ab], n_pos, hip.UPWGRAD_CHAIN))
    report(label, "d_short_bias", np.abs(got["short_bias"].astype(np.float64) - t["d_short_bias"].astype(np.float32).astype(np.float64)),
           R.ulp32(t["d_short_bias"]))


@pytest.mark.parametrize("name", F.CASES)
def test_64_32_32_gives_the_bytes_of_the_older_entry(name):
    """convup_wgrad forwards to the kernel of convupn_wgrad: both must still give the bytes that the 96 -> 32 kernel gave
    while it was a kernel of its own (tests/make_grad_fold_digests.py), for every case, cap and output, and so the bytes of
    each other."""
    want = F.load()
    old = F.convup_outputs(name, last_block.convup_wgrad)
    new = F.convup_outputs(name, dec2_block.convupn_wgrad)
    keys = [k for k in want if k.startswith(f"convup/{name}/")]
    assert sorted(old) == sorted(new) == sorted(keys) and len(keys) == len(KEYS) * len(F.CONVUP_CAPS) + 2
    for k in keys:
        assert same_bytes(old[k], new[k]), (k, mismatch(new[k], old[k]))
        assert F.digest(old[k]) == want[k], (k, "convup entry: not the bytes of the 96 -> 32 kernel")
        assert F.digest(new[k]) == want[k], (k, "convupn entry: not the bytes of the 96 -> 32 kernel")


def test_a_nearest_upsample_that_is_not_the_half_map_is_refused(monkeypatch):
    from v2ce_toolbox_amd import v2ce_3d
    z = inputs((2, 3, 5, 7), (128, 64, 64), False)
    monkeypatch.setattr(v2ce_3d, "_nearest_is_half", lambda n_in, n_out: False)
    with pytest.raises(ValueError, match="does not read its source"):
        dec2_block.convupn_wgrad(z["c16_x0"], z["c16_x1"], z["c16_g1"], z["c16_gd"])


def test_the_checked_entry_refuses_what_the_header_refuses():
    shape, triple = (1, 2, 3, 70), (128, 64, 64)
    z = inputs(shape, triple, False)
    x0, x1, g1, gd = z["c16_x0"], z["c16_x1"], z["c16_g1"], z["c16_gd"]
    wg = dec2_block.convupn_wgrad
    with pytest.raises(ValueError, match="want"):
        wg(x0, x1, g1, gd, want=())
    with pytest.raises(ValueError, match="want"):
        wg(x0, x1, g1, gd, want=("short", "short"))
    with pytest.raises(ValueError, match="needs g1"):
        wg(x0, x1, None, gd)
    with pytest.raises(ValueError, match="need gd"):
        wg(x0, x1, g1, None)
    with pytest.raises(ValueError, match="max_workgroups"):
        wg(x0, x1, g1, gd, max_workgroups=-1)
    with pytest.raises(hip.V2ceHipError, match="HIP device"):
        wg(x0.cpu(), x1, g1, gd)
    with pytest.raises(ValueError, match="float32"):
        wg(x0, x1, g1.double(), gd)
    three = torch.zeros((1, 2, 3, 3, 96, 16), device=DEV)               # 48 channels
    three.lw = 70
    with pytest.raises(ValueError, match="channels-last-16"):
        wg(x0, three, g1, gd)
    with pytest.raises(ValueError, match="channels-last-16"):
        wg(x0, x1, three, gd)
    half = inputs(shape, (64, 64, 32), False)
    with pytest.raises(ValueError, match="must match g1"):
        wg(x0, x1, g1, half["c16_gd"])                                  # gd with other planes than g1
    other = G.to_c16(z["x1"][:, :, :, :, :69].contiguous(), 96)
    with pytest.raises(ValueError, match="must match"):
        wg(x0, other, g1, gd)                                           # another .lw: x0 no longer fits
    with pytest.raises(ValueError, match="must match x1"):
        wg(x0, x1, G.to_c16(z["g1"][:, :, :, :, :69].contiguous(), 96), gd)
    tall = G.to_c16(torch.zeros((1, 128, 2, 3, 35), device=DEV), 35)     # h0 = 3 for h = 3
    with pytest.raises(ValueError, match="must match x1"):
        wg(tall, x1, g1, gd)
    with pytest.raises(ValueError, match="16-byte"):
        t = torch.zeros(gd.numel() + 1, device=DEV)[1:].view(gd.shape)
        t.lw = 70
        wg(x0, x1, g1, t)
    with pytest.raises(ValueError, match="out holds"):
        wg(x0, x1, g1, gd, want=("weight",), out={"short": torch.zeros((64, 192), device=DEV)})
    with pytest.raises(ValueError, match="elements"):
        wg(x0, x1, g1, gd, out={"weight": torch.zeros((32, 192, 3, 3, 3), device=DEV)})
    with pytest.raises(ValueError, match="overlaps"):
        wg(x0, x1, g1, gd, out={"short_bias": gd.view(-1)[:64]})
    torch.cuda.synchronize()
