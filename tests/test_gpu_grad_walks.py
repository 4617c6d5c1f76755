"""The five gradient kernels on full-grid tile walks against f64 truths computed on the device (tests/grad_walk_ref.py):
v2ce_pred_head_grads, v2ce_conv32_wgrad, v2ce_conv32_dgrad, v2ce_convup_wgrad and v2ce_convup_dgrad through their checked
Python entries, at shapes where the default grid is at its cap and every workgroup walks an uneven share of the tiles
(tests/test_grad_walk_cpu.py proves the table's properties):

  wide  [3, 5, 75, 131]   1710 tiles: shares of 6-7 (256 workgroups) and 20-21 (85 shares); the head walks 1152 tiles in
                          shares of 2-3 (512 workgroups).  Odd H, W = 2 * 64 + 3: one-row and three-column last tiles;
                          shares start and end inside frames, rows of tiles and sequences.  All five kernels.
  deep  [3, 8, 353, 65]   8496 tiles: shares of 33-34 for conv32_wgrad (one flush of the f32 chain, then 1-2 tiles) and of
                          99-100 for convup_wgrad (three flushes, then 3-4 tiles).  The two weight-gradient kernels.

Check A, exact.  Integers 1 .. 3 in every value tensor, a normal y with signed zeros for the mask.  Every sum the kernels
form is an integer below 2^24, so f32 chains, f64 partials and the store are exact: every element of every output must
equal the f64 truth rounded to f32, bit for bit, with zero tolerance, at the default grid and again at max_workgroups = 97
(whose bytes must be the default grid's).  All terms are positive: a tile that is dropped, repeated, read across a b or l
boundary or paired with the wrong tap changes a sum and cannot cancel.  Outputs go in filled with NaN where the entry takes
them, so an element that is never written shows too.  (v2ce_pred_head_grads takes no max_workgroups: its second run checks
the bytes from run to run.)

Check B, contract.  Standard normals; each output within the bound its header states (the bound functions of the golden
tests: wgrad_bound with N and the chain constant, dgrad_bound with 864 terms or V2CE_UPDGRAD_TERMS times the element's
output positions, one f32 ulp for the f64-throughout outputs), the worst element printed as a fraction of its bound.

What this pins down: share arithmetic, halo reuse between tiles, the flush and the `stored` flag, the finish kernels' loops
over 256 / 255 / 512 partial slots, the workspace at its largest.  Check B proves the rounding contract at scale; only
check A detects a lost tile (on normal data at the deep row one tile moves an element by a fraction of its bound).
The chain length, the f64 sums above it, the f32 products and the per-element arithmetic are pinned down by the adversarial
data of tests/test_gpu_grad_probes.py."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_walk_ref as G
from tests import last_block_dgrad_ref as BD
from tests import last_block_ref as BR
from tests import last_conv_dgrad_ref as CD
from tests import last_conv_ref as CR
from v2ce_toolbox_amd import hip, last_block, last_conv, pred_head

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = {True: 101, False: 202}
CONV_CASES = [(op, "wide") for op in ("conv32_wgrad", "conv32_dgrad", "convup_wgrad", "convup_dgrad")] + \
             [("conv32_wgrad", "deep"), ("convup_wgrad", "deep")]
# kernel output -> key of the truth
NAMES = {"conv32_wgrad": {"weight": "d_weight", "shift": "d_shift"}, "conv32_dgrad": {"x": "d_x", "res": "d_res"},
         "convup_wgrad": {"weight": "d_weight", "short": "d_short", "short_bias": "d_short_bias"},
         "convup_dgrad": {"x0": "d_x0", "x1": "d_x1"},
         "pred_head_grads": {"weight": "d_weight", "bias": "d_bias", "feat": "d_feat"}}


@functools.lru_cache(maxsize=None)
def inputs(row, exact):
    """The convolution kernels' inputs in the reference's layouts on the device, and their channels-last-16 forms at the
    activation pitch with NaN in the padding columns (prefix c16_)."""
    shape = G.WALKS[row]
    z = {k: v.to(DEV) for k, v in G.walk_inputs(shape, exact, SEEDS[exact]).items()}
    W = shape[3]
    for k in ("x", "y", "upstream", "x1", "g1", "gd"):
        z["c16_" + k] = G.to_c16(z[k], G.pitch_of(W))
    z["c16_x0"] = G.to_c16(z["x0"], G.pitch_of((W + 1) // 2))
    return z


@functools.lru_cache(maxsize=None)
def head_inputs(row, exact, cout):
    shape = G.WALKS[row]
    z = {k: v.to(DEV) for k, v in G.head_inputs(shape, exact, SEEDS[exact] + cout, cout).items()}
    z["c16_feat"] = G.to_c16(z["feat"], G.pitch_of(shape[3]))
    z["dense_y"], z["dense_up"] = G.to_dense(z["y_head"]), G.to_dense(z["up_head"])
    return z


@functools.lru_cache(maxsize=None)
def truth(op, row, exact, cout=None):
    """The f64 truth on the device, computed once per (kernel, row, data)."""
    if op == "pred_head_grads":
        z = head_inputs(row, exact, cout)
        return G.pred_head_grads(z["feat"], z["y_head"], z["up_head"], z["w_head"])
    z = inputs(row, exact)
    if op == "conv32_wgrad":
        return G.conv32_wgrad(z["x"], z["y"], z["upstream"])
    if op == "conv32_dgrad":
        return G.conv32_dgrad(z["weight"], z["y"], z["upstream"])
    if op == "convup_wgrad":
        return G.convup_wgrad(z["x0"], z["x1"], z["g1"], z["gd"])
    t = G.convup_dgrad(z["weight_up"], z["short"], z["g1"], z["gd"])
    del t["d_X"]
    return t


def nan_like(t):
    return torch.full_like(t, float("nan"))


def run(op, row, exact, max_workgroups=0, cout=None):
    """One call of the checked Python entry -> {name: the whole output tensor on the device}."""
    if op == "pred_head_grads":
        z = head_inputs(row, exact, cout)
        g = pred_head.pred_head_grads(z["c16_feat"], z["dense_y"], z["dense_up"], z["w_head"], want=("weight", "bias", "feat"),
                                      out={"feat": nan_like(z["c16_feat"])})
    else:
        z = inputs(row, exact)
        kw = {"max_workgroups": max_workgroups}
        if op == "conv32_wgrad":
            g = last_conv.conv32_wgrad(z["c16_x"], z["c16_y"], z["c16_upstream"], **kw)
        elif op == "conv32_dgrad":
            g = last_conv.conv32_dgrad(z["weight"], z["c16_y"], z["c16_upstream"],
                                       out={"x": nan_like(z["c16_upstream"]), "res": nan_like(z["c16_upstream"])}, **kw)
        elif op == "convup_wgrad":
            g = last_block.convup_wgrad(z["c16_x0"], z["c16_x1"], z["c16_g1"], z["c16_gd"], **kw)
        else:
            g = last_block.convup_dgrad(z["weight_up"], z["short"], z["c16_g1"], z["c16_gd"],
                                        out={"x0": nan_like(z["c16_x0"]), "x1": nan_like(z["c16_g1"])}, **kw)
    torch.cuda.synchronize()
    assert set(g) == set(NAMES[op])
    return g


def logical(op, name, t, row):
    """The output in the truth's layout: the logical columns of a channels-last-16 tensor, a weight as it is."""
    W = G.WALKS[row][3]
    if t.dim() == 6:
        return G.from_c16(t, (W + 1) // 2 if name == "x0" else W)
    return t


def padding_of(name, t, row):
    W = G.WALKS[row][3]
    return t[:, :, :, :, ((W + 1) // 2 if name == "x0" else W):, :]


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def describe_mismatch(got, want):
    """The element pattern of a failed exact check: how many, where the first ones are, by how much."""
    bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
    spread = {d: sorted(set(bad[:, d].tolist()))[:12] for d in range(bad.shape[1])}
    return f"{bad.shape[0]} of {got.numel()} elements differ; first (index, got, want): {first}; indices per dim: {spread}"


def check_exact(op, row, cout=None):
    t = truth(op, row, True, cout)
    own = run(op, row, True, cout=cout)
    for name, key in NAMES[op].items():
        got, want = logical(op, name, own[name], row), t[key].to(torch.float32)
        assert torch.equal(want.to(torch.float64), t[key]) and float(t[key].max()) < 2 ** 24      # the truth is an f32
        assert float(t[key].max()) > 0
        assert got.shape == want.shape, (op, name, tuple(got.shape))
        assert not torch.isnan(got).any(), (op, row, name, "NaN: an element was not written, or a padding column was read")
        assert same_bytes(got, want), (op, row, name, describe_mismatch(got, want))
        if own[name].dim() == 6:
            pad = padding_of(name, own[name], row)
            assert pad.numel() > 0
            if op == "pred_head_grads":                              # the head never writes d_feat's padding columns
                assert torch.isnan(pad).all(), (op, name)
            else:
                assert not pad.any(), (op, row, name, "padding columns must be zeros")
    # a grid of another size (the head takes none: the same grid again) gives the same bytes
    other = run(op, row, True, max_workgroups=G.OTHER_GRID, cout=cout)
    for name in NAMES[op]:
        a, b = (logical(op, name, v[name], row) if op == "pred_head_grads" else v[name] for v in (own, other))
        assert same_bytes(a, b), (op, row, name, f"max_workgroups={G.OTHER_GRID}", describe_mismatch(a, b))


def report(label, name, err, bound):
    frac = float((err / bound).max())
    print(f"{label}: {name}: max error {float(err.max()):.3e}, {frac:.3g} of its bound")
    assert np.all(err <= bound), (label, name, float(err.max()), frac)


def one_ulp(label, name, got, want):
    """An f64-throughout output: within one f32 ulp of the truth rounded to f32."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    report(label, name, err, CR.ulp32(want))


def check_contract(op, row, cout=None):
    t = {k: v.cpu().numpy() for k, v in truth(op, row, False, cout).items()}
    own = run(op, row, False, cout=cout)
    got = {}
    for name in NAMES[op]:
        v = logical(op, name, own[name], row)
        assert not torch.isnan(v).any(), (op, row, name)
        got[name] = v.cpu().numpy()
    n = int(np.prod(G.WALKS[row]))
    label = f"{op} {row}" + (f" cout {cout}" if cout else "")
    err = lambda name, key: np.abs(got[name].astype(np.float64) - t[key])
    if op == "conv32_wgrad":
        report(label, "d_weight", err("weight", "d_weight"), CR.wgrad_bound(t["d_weight"], t["abs_weight"], n, hip.WGRAD_CHAIN))
        one_ulp(label, "d_shift", got["shift"], t["d_shift"])
    elif op == "conv32_dgrad":
        report(label, "d_x", err("x", "d_x"), CD.dgrad_bound(t["abs_x"], hip.DGRAD_TERMS))
        assert np.array_equal(got["res"].view(np.int32), t["d_res"].astype(np.float32).view(np.int32))     # a copy
    elif op == "convup_wgrad":
        report(label, "d_weight", err("weight", "d_weight"), BR.wgrad_bound(t["d_weight"], t["abs_weight"], n, hip.UPWGRAD_CHAIN))
        report(label, "d_short", err("short", "d_short"), BR.wgrad_bound(t["d_short"], t["abs_short"], n, hip.UPWGRAD_CHAIN))
        one_ulp(label, "d_short_bias", got["short_bias"], t["d_short_bias"])
    elif op == "convup_dgrad":
        report(label, "d_x1", err("x1", "d_x1"), BD.dgrad_bound(t["abs_x1"], hip.UPDGRAD_TERMS))
        assert set(np.unique(t["n_x0"])) == {1.0, 2.0, 4.0}
        report(label, "d_x0", err("x0", "d_x0"), BD.dgrad_bound(t["abs_x0"], hip.UPDGRAD_TERMS * t["n_x0"]))
    else:
        one_ulp(label, "d_weight", got["weight"].reshape(-1, 32), t["d_weight"])
        one_ulp(label, "d_bias", got["bias"], t["d_bias"])
        one_ulp(label, "d_feat", got["feat"], t["d_feat"])
    for name in NAMES[op]:
        if own[name].dim() == 6 and op != "pred_head_grads":
            assert not padding_of(name, own[name], row).any(), (op, row, name)


@pytest.mark.parametrize("op,row", CONV_CASES)
def test_integer_walk_is_bit_exact_at_the_default_grid_and_at_97(op, row):
    check_exact(op, row)


@pytest.mark.parametrize("cout", G.HEAD_COUTS)
def test_integer_walk_of_the_head_is_bit_exact(cout):
    check_exact("pred_head_grads", "wide", cout)


@pytest.mark.parametrize("op,row", CONV_CASES)
def test_normal_walk_is_inside_the_contract_bound(op, row):
    check_contract(op, row)


@pytest.mark.parametrize("cout", G.HEAD_COUTS)
def test_normal_walk_of_the_head_is_inside_one_ulp(cout):
    check_contract("pred_head_grads", "wide", cout)
