"""The prediction-head kernels (v2ce_pred_head_fwd / v2ce_pred_head_grads through pred_head.py) on the GPU against the
reference layer's own f64 results (tests/golden/.predhead/) and the numpy restatement (tests/pred_head_ref.py).

Bounds (from the header's arithmetic, not from what the kernels give): every output is an f64 sum rounded once, so
  y, d_feat, d_bias   within 1 f32 ulp of (float)ref64 (a few f64 roundings can move a sum across one f32 tie);
  d_weight            within ulp32 + N 2^-52 abs_terms, N the number of positions and abs_terms the sum of |terms| of
                      the element: the f64 summation-order bound of N additions.
The same bounds hold against the restatement evaluated on the device's own y."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from tests import pred_head_ref as R
from v2ce_toolbox_amd import hip, pred_head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", ".predhead", "*.npz")))
name_of = lambda p: os.path.basename(p)[:-4]
TILE, MAX_GRID = 128, 512                    # csrc/pred_head.hip: positions per tile, workgroups of the gradient kernel


def offset_copy(a, elems):
    """A device copy of `a` whose first element sits `elems` floats past an allocation's start."""
    a = np.ascontiguousarray(a, np.float32)
    flat = torch.zeros(a.size + elems + 64, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 256 == 0
    v = flat[elems:elems + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def device_inputs(feat, weight, bias, upstream, pitch=None, shifted=False):
    """The kernels' tensors for inputs in the reference's layouts; padding columns hold NaN.  shifted: base pointers 16
    bytes (channels-last-16) and 4 bytes (dense) past a 256-byte boundary."""
    W = feat.shape[-1]
    pitch = R.pitch_of(W) if pitch is None else pitch
    f = offset_copy(R.to_c16(feat, pitch), 4 if shifted else 0)
    f.lw, f.c16 = W, True
    w = torch.from_numpy(np.ascontiguousarray(weight, np.float32)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda()
    u = offset_copy(R.to_dense(upstream), 1 if shifted else 0)
    return f, w, b, u


def run_device(feat, weight, bias, upstream, want=("weight", "bias", "feat"), pitch=None, shifted=False, y_from=None):
    """-> dict y [B, Cout, L, H, W], d_weight [Cout, 32], d_bias, d_feat [B, 32, L, H, W] (numpy f32) and d_feat_c16, feat_c16."""
    W = feat.shape[-1]
    f, w, b, u = device_inputs(feat, weight, bias, upstream, pitch, shifted)
    if shifted:
        B, L, H, cout = f.shape[0], f.shape[1], f.shape[3], w.shape[0]
        y = offset_copy(np.zeros((B, L, cout, H, W), np.float32), 1)
        pred_head.pred_head_forward(f, w, b, out=y)
    else:
        y = pred_head.pred_head_forward(f, w, b)
    out = {}
    if "feat" in want:                       # the padding columns of d_feat are the caller's: NaN, to see them kept
        df = torch.full_like(f, float("nan")) if not shifted else offset_copy(np.full(tuple(f.shape), np.nan, np.float32), 4)
        out["feat"] = df
    g = pred_head.pred_head_grads(f, y if y_from is None else y_from, u, w, want=want, out=out)
    torch.cuda.synchronize()
    res = {"y": R.from_dense(y.cpu().numpy()), "feat_c16": f.cpu().numpy(), "y_dev": y}
    if "weight" in g:
        res["d_weight"] = g["weight"].cpu().numpy().reshape(-1, 32)
    if "bias" in g:
        res["d_bias"] = g["bias"].cpu().numpy()
    if "feat" in g:
        res["d_feat_c16"] = g["feat"].cpu().numpy()
        res["d_feat"] = R.from_c16(res["d_feat_c16"], W)
    return res


def check_against(got, want_y, want_g, n_pos, label):
    """The bounds of the module docstring; want_*: f64 truth in the reference's layouts."""
    def within(name, a, truth, slack=0.0):
        t32 = truth.astype(np.float32).astype(np.float64)
        err = np.abs(a.astype(np.float64) - t32)
        bound = R.ulp32(truth) + slack
        worst = float((err / bound).max()) if err.size else 0.0
        print(f"{label}: {name}: max error {err.max() if err.size else 0.0:.3e}, {worst:.3f} of its bound")
        assert np.all(err <= bound), (label, name, float(err.max()), worst)
    within("y", got["y"], want_y)
    if "d_feat" in got:
        within("d_feat", got["d_feat"], want_g["d_feat"])
    if "d_bias" in got:
        within("d_bias", got["d_bias"], want_g["d_bias"])
    if "d_weight" in got:
        within("d_weight", got["d_weight"], want_g["d_weight"], n_pos * 2.0 ** -52 * want_g["abs_weight"])


def restated(feat, weight, bias, upstream, y_dev32):
    """The restatement on the device's own output: (y truth, gradient truth)."""
    return R.forward(feat, weight, bias), R.grads(feat, y_dev32, upstream, weight)


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_kernels_match_the_reference_layer_and_the_restatement(path):
    z = np.load(path)
    feat, weight, bias, up = z["feat"], z["weight"], z["bias"], z["upstream"]
    got = run_device(feat, weight, bias, up)
    n = R.positions(feat)
    ref = {"d_weight": z["ref64_d_weight"], "d_bias": z["ref64_d_bias"], "d_feat": z["ref64_d_feat"],
           "abs_weight": z["abs_terms_d_weight"]}
    check_against(got, z["ref64_y"], ref, n, name_of(path) + " vs reference")
    check_against(got, *restated(feat, weight, bias, up, got["y"]), n, name_of(path) + " vs restatement")
    # the padding columns of the features were NaN and were not read; those of d_feat were not written
    W = feat.shape[-1]
    if got["feat_c16"].shape[4] > W:
        assert name_of(path) == "b1_l2_3x70" and got["feat_c16"].shape[4] == 96
        assert np.isnan(got["feat_c16"][..., W:, :]).all() and np.isnan(got["d_feat_c16"][..., W:, :]).all()
    assert not np.isnan(got["d_feat_c16"][..., :W, :]).any() and not np.isnan(got["y"]).any()


def random_case(seed, B, L, H, W, cout=20):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((B, 32, L, H, W)).astype(np.float32)
    feat[rng.random(feat.shape) < 0.2] = 0.0
    weight = (rng.standard_normal((cout, 32, 1, 1, 1)) * 0.2).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    up = rng.standard_normal((B, cout, L, H, W)).astype(np.float32)
    return feat, weight, bias, up


# [1, 1, 3, 43]: 129 positions, one whole 128-position tile and a second with a single position; two workgroups.
# [1, 2, 7, 19]: 266 positions, tiles that straddle rows and a frame boundary, ragged last tile.
# [1, 2, 190, 346]: 131 480 positions = 1027.2 tiles on the 512 workgroups of the gradient kernel: every workgroup walks 2
# or 3 tiles (more than one, 346-wide rows at pitch 352) and the last tile holds 24 positions.  The issue's
# [1, 2, 40, 346] (216.3 tiles) would give every workgroup a single tile on this grid.
SHAPES = {"one_past_a_tile": (1, 1, 3, 43, 20), "ragged_rows": (1, 2, 7, 19, 20), "multi_tile_walk": (1, 2, 190, 346, 20),
          "cout_9": (2, 1, 5, 13, 9), "cout_24": (1, 1, 6, 11, 24)}


@pytest.mark.parametrize("name", SHAPES, ids=list(SHAPES))
def test_more_shapes_match_the_restatement(name):
    B, L, H, W, cout = SHAPES[name]
    case = random_case(sorted(SHAPES).index(name) + 90, B, L, H, W, cout)
    n = B * L * H * W
    if name == "multi_tile_walk":
        tiles = -(-n // TILE)
        assert tiles > 2 * MAX_GRID and tiles < 3 * MAX_GRID and n % TILE not in (0,) and R.pitch_of(W) == 352
    got = run_device(*case)
    check_against(got, *restated(*case, got["y"]), n, name)
    assert np.isnan(got["d_feat_c16"][..., W:, :]).all()


@functools.lru_cache(maxsize=None)
def base_case():
    return random_case(7, 2, 2, 5, 70)                              # 1 400 positions at pitch 96: 11 tiles


def test_two_runs_give_identical_bytes():
    a, b = run_device(*base_case()), run_device(*base_case())
    for k in ("y", "d_weight", "d_bias", "d_feat_c16"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_offset_base_pointers():
    a = run_device(*base_case())
    s = run_device(*base_case(), shifted=True)
    for k in ("y", "d_weight", "d_bias", "d_feat_c16"):
        assert np.array_equal(a[k].view(np.uint32), s[k].view(np.uint32)), k


def test_want_subsets_write_only_what_was_asked_and_match_the_full_call():
    full = run_device(*base_case())
    keys = {"weight": "d_weight", "bias": "d_bias", "feat": "d_feat_c16"}
    for want in (("weight",), ("bias",), ("feat",), ("weight", "bias"), ("bias", "feat"), ("weight", "feat")):
        got = run_device(*base_case(), want=want)
        assert {k for k in keys.values() if k in got} == {keys[w] for w in want}, want
        for w in want:
            assert np.array_equal(got[keys[w]].view(np.uint32), full[keys[w]].view(np.uint32)), (want, w)
    # an output that was not asked for is not touched: poisoned buffers passed next to a one-output call stay poisoned
    f, w, b, u = device_inputs(*base_case())
    y = pred_head.pred_head_forward(f, w, b)
    L = hip.lib()
    B, Lq, _, H, pitch, _ = f.shape
    nb = L.v2ce_pred_head_grads_workspace_bytes(B, Lq, 20, H, f.lw, pitch)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dw = torch.full((20, 32), 7.0, device="cuda")
    assert L.v2ce_pred_head_grads(f.data_ptr(), y.data_ptr(), u.data_ptr(), w.data_ptr(), B, Lq, 20, H, f.lw, pitch,
                                  None, None, None, ws.data_ptr(), nb, hip.stream_ptr()) == -1      # no output requested
    hip.check(L.v2ce_pred_head_grads(f.data_ptr(), y.data_ptr(), u.data_ptr(), w.data_ptr(), B, Lq, 20, H, f.lw, pitch,
                                     dw.data_ptr(), None, None, ws.data_ptr(), nb, hip.stream_ptr()), "v2ce_pred_head_grads")
    assert np.array_equal(dw.cpu().numpy().view(np.uint32), full["d_weight"].view(np.uint32))


def test_nan_in_upstream_propagates_and_nan_in_y_gives_zero():
    feat, weight, bias, up = (a.copy() for a in base_case())
    clean = run_device(feat, weight, bias, up)
    y = clean["y"]
    # an active unit with a NaN upstream: its d_bias, its row of d_weight and its position's d_feat become NaN
    idx = tuple(np.argwhere(y > 0)[17])
    b, co, l, h, w = idx
    up[idx] = np.nan
    got = run_device(feat, weight, bias, up)
    assert np.isnan(got["d_bias"][co]) and not np.isnan(np.delete(got["d_bias"], co)).any()
    assert np.isnan(got["d_weight"][co]).all() and not np.isnan(np.delete(got["d_weight"], co, axis=0)).any()
    assert np.isnan(got["d_feat"][b, :, l, h, w]).all()
    rest = got["d_feat"].copy()
    rest[b, :, l, h, w] = 0
    assert not np.isnan(rest).any()
    # an inactive unit with a NaN upstream: masked, nothing changes
    up = base_case()[3].copy()
    off = tuple(np.argwhere(y == 0)[5])
    up[off] = np.nan
    got = run_device(feat, weight, bias, up)
    for k in ("d_weight", "d_bias", "d_feat_c16"):
        assert np.array_equal(got[k].view(np.uint32), clean[k].view(np.uint32)), k
    # a NaN in y itself counts as inactive (torch's relu backward: y > 0 is false)
    f, wt, bs, u = device_inputs(*base_case())
    ybad = clean["y_dev"].clone()
    flat = R.to_dense(y).reshape(-1)
    k = int(np.flatnonzero(flat > 0)[3])
    ybad.view(-1)[k] = float("nan")
    g = pred_head.pred_head_grads(f, ybad, u, wt, want=("weight", "bias", "feat"))
    yz = clean["y_dev"].clone()
    yz.view(-1)[k] = 0.0
    gz = pred_head.pred_head_grads(f, yz, u, wt, want=("weight", "bias", "feat"))
    for n in ("weight", "bias"):
        assert torch.equal(g[n], gz[n]) and not torch.isnan(g[n]).any(), n
    W = f.lw
    assert torch.equal(g["feat"][..., :W, :], gz["feat"][..., :W, :])


def test_python_refusals_on_the_device():
    f, w, b, u = device_inputs(*base_case())
    y = pred_head.pred_head_forward(f, w, b)
    with pytest.raises(ValueError, match="float32"):
        pred_head.pred_head_forward(f, w.double(), b)
    with pytest.raises(ValueError, match="contiguous"):
        pred_head.pred_head_grads(f, y.transpose(3, 4), u, w)
    with pytest.raises(ValueError, match=r"\[b, l, cout, h, w\]"):
        pred_head.pred_head_grads(f, y[:1], u, w)
    with pytest.raises(ValueError, match="overlaps"):
        pred_head.pred_head_grads(f, y, u, w, want=("weight",), out={"weight": w})
    with pytest.raises(ValueError, match="overlaps"):
        pred_head.pred_head_forward(f, w, b, out=f.view(-1)[:y.numel()].view(y.shape))
    with pytest.raises(ValueError, match="channels-last-16"):
        pred_head.pred_head_forward(torch.zeros(1, 2, 2, 4, 5, 8, device="cuda"), w, b)
    with pytest.raises(ValueError, match="32"):
        pred_head.pred_head_forward(f, torch.zeros(20, 16, device="cuda"), b)
