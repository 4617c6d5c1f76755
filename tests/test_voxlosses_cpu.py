"""CPU side of the stage-1 loss terms (v2ce_voxlosses / losses.py): the numpy restatement (tests/voxlosses_ref.py)
against the reference's own results (tests/golden/.voxlosses/), what each fixture exercises, the argument refusals of
the C ABI and of losses.py that need no GPU.

Bounds: against the reference run on .double() inputs (ref64) the f64 restatement agrees to 1e-10 relative; against
the reference as it runs (ref, f32) a value may be no farther away than the reference is from its own f64 run, plus
the f32 rounding of the result (1e-6 relative)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import voxlosses_ref as R
from v2ce_toolbox_amd import hip, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".voxlosses")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
FULL = os.path.join(GOLD, "full_b1_l16_260x346.npz")
ARRAY_GOLDENS = [p for p in GOLDENS if p != FULL]
EF_KEY = {"only_c": "only_c", "cl": "cl", "c+cl": "c_cl"}
ALL_LOSS = ("pyramid", "pt", "ef", "ef_splitp", "match", "compensation", "norml1", "norml2")
DEFAULT_LOSS = ("pyramid", "ef", "ef_splitp", "compensation")
name_of = lambda p: os.path.basename(p)[:-4]


def specs(z):
    """(suffix of the golden's keys, keywords of calculate_loss, which value, second stage?) for every stored value."""
    out = []
    for ef_type, ek in EF_KEY.items():
        for base in (False, True):
            kw = dict(loss=ALL_LOSS, ef_type=ef_type, add_base_loss=base)
            out.append((f"ef_both_{ek}", kw, "ef_loss", False))
            out.append((f"pyramid_base{int(base)}", kw, "pyramid_loss", False))
            out.append((f"loss_all_{ek}_base{int(base)}", kw, "loss", False))
        for kind in ("ef", "ef_splitp"):
            out.append((f"{kind}_only_{ek}", dict(loss=(kind,), ef_type=ef_type), "ef_loss", False))
    for k in ("pt_loss", "match", "compensation", "norml1", "norml2"):
        out.append((k, dict(loss=ALL_LOSS), k, False))
    out.append(("loss_default", dict(loss=DEFAULT_LOSS), "loss", False))
    if "pred2" in z.files:
        out.append(("stages_loss", dict(loss=ALL_LOSS), "loss", True))
        for k in ("ef_loss", "pyramid_loss", "pt_loss", "match", "compensation", "norml1", "norml2"):
            out.append((f"stages_{k}", dict(loss=ALL_LOSS), k, True))
    return out


def check_two_sided(got, z, suffix, what=""):
    """No farther from the reference than the reference is from its own f64 run, plus f32 rounding of the result."""
    r32, r64 = float(z[f"ref_{suffix}"]), float(z[f"ref64_{suffix}"])
    assert abs(got - r32) <= abs(r32 - r64) + 1e-6 * abs(r64), (what, suffix, got, r32, r64)


def golden_inputs(path):
    z = np.load(path)
    if path != FULL:
        return z, z["pred"], z["gt"], (z["pred2"] if "pred2" in z.files else None)
    from v2ce_toolbox_amd import synth
    L, H, W = int(z["L"]), int(z["H"]), int(z["W"])
    mk = lambda seed: synth.synthetic_voxels(L, H, W, seed=int(seed), regime=str(z["regime"])).reshape(1, L, 20, H, W)
    p, g = mk(z["pred_seed"]), mk(z["gt_seed"])
    assert p.astype(np.float64).sum() == float(z["pred_sum"]) and g.astype(np.float64).sum() == float(z["gt_sum"])
    return z, p, g, None


def test_goldens_present_and_small():
    assert [name_of(p) for p in GOLDENS] == sorted(
        ["at_threshold", "b1_l1_8x8", "b1_l1_9x15", "b1_l4_16x24", "b2_l3_11x13", "b3_l2_8x70",
         "full_b1_l16_260x346", "zero_gt"])
    for p in GOLDENS:
        assert os.path.getsize(p) <= 300 * 1024, p


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_restatement_matches_the_reference(path):
    z, p, g, p2 = golden_inputs(path)
    one = [R.total(R.batch_stats(p, g))]
    assert one[0]["match_low"] == 0                                  # the condition on every fixture
    two = one + [R.total(R.batch_stats(p2, g))] if p2 is not None else None
    for suffix, kw, pick, staged in specs(z):
        total, d = R.loss_values(two if staged else one, **kw)
        got = total if pick == "loss" else d[pick]
        r64 = float(z[f"ref64_{suffix}"])
        assert abs(got - r64) <= 1e-10 * abs(r64), (suffix, got, r64)
        check_two_sided(got, z, suffix)


@pytest.mark.parametrize("path", ARRAY_GOLDENS, ids=name_of)
def test_fixtures_exercise_their_terms(path):
    z = np.load(path)
    p, g = z["pred"], z["gt"]
    name = name_of(path)
    for k in ("pyramid_base0", "pt_loss", "ef_both_c_cl", "ef_only_cl", "ef_splitp_only_only_c", "match", "compensation",
              "norml1", "norml2", "loss_default"):
        if k == "match" and p.shape[1] == 1:
            assert float(z["ref_match"]) == 0                       # a softmax over one frame: log 1
            continue
        assert float(z[f"ref_{k}"]) > 0, (name, k)
    s = R.total(R.batch_stats(p, g))
    assert all(s["pyr_sq_sum"] > 0) and all(s["temporal_sq_sum"] > 0) and all(s["ef_sq_sum"] > 0)
    L, H, W = p.shape[1], p.shape[3], p.shape[4]
    if name == "b1_l1_8x8":
        assert s["pyr_n"][2] == 2 and s["temporal_n"][0] == 2 * 64 * 4          # one k = 8 window per polarity; 4 of size 3
    if name == "b1_l1_9x15":
        assert (H % 8, W % 8, H % 2, W % 2) == (1, 7, 1, 1)
    if name == "b2_l3_11x13":
        assert L % 2 == 1 and (10 * L) % 4 and (10 * L) % 8
    if name == "b1_l4_16x24":
        assert 10 * L == 40 and s["pyr_n"][2] == 2 * 5 * 2 * 3
    if name == "b3_l2_8x70":
        assert W > 64
    if name == "zero_gt":
        assert not g.any()
        assert (np.argmax(g, axis=1) == 0).all()                    # every column of gt over l is a tie: index 0
        assert ((g > np.float32(0.01)).sum(axis=(2, 3)) == 0).all()  # every gt count clamps to 1
    if name == "at_threshold":
        thr = np.float32(0.01)
        up = np.nextafter(thr, np.float32(1))
        for a in (p, g):
            assert (a == thr).sum() > 50 and (a == up).sum() > 50


def test_temporal_pool_of_size_3_drops_or_pads_the_last_plane():
    rng = np.random.default_rng(3)
    for D in (5, 6, 7, 8, 9, 10):
        p, g = rng.random((D, 2, 3), dtype=np.float32), rng.random((D, 2, 3), dtype=np.float32)
        s = R.volume_stats(p, g, pyramid=False)
        pool = torch.nn.AvgPool1d(3, stride=3, padding=1)
        t = lambda a: pool(torch.from_numpy(a).double().reshape(D, 6).T[None])
        want = ((t(p) - t(g)) ** 2)
        assert s["temporal_n"][0] == want.numel() == 6 * ((D - 1) // 3 + 1)
        assert abs(s["temporal_sq_sum"][0] - float(want.sum())) <= 1e-12 * float(want.sum())


def test_abi_refusals_without_gpu():
    L = hip.lib()
    every = sum(losses.TERMS.values())
    assert L.v2ce_voxlosses_workspace_bytes(4, 16, 20, 260, 346, every) > 0
    assert L.v2ce_voxlosses_workspace_bytes(1, 1, 20, 8, 8, every) > 0
    assert L.v2ce_voxlosses_workspace_bytes(1, 1, 18, 8, 8, every) == 0                   # C != 20
    assert L.v2ce_voxlosses_workspace_bytes(1, 1, 20, 7, 8, hip.VOXLOSSES_PYRAMID) == 0    # the 8-wide window must fit
    assert L.v2ce_voxlosses_workspace_bytes(1, 1, 20, 7, 8, every & ~hip.VOXLOSSES_PYRAMID) > 0
    assert L.v2ce_voxlosses_workspace_bytes(1, 1, 20, 8, 8, 64) == 0                      # unknown term bit
    assert L.v2ce_volume_losses_workspace_bytes(2, 7, 8, 8, hip.VOXLOSSES_PYRAMID) == 0
    assert L.v2ce_volume_losses_workspace_bytes(2, 4, 8, 8, hip.VOXLOSSES_TEMPORAL) == 0
    assert L.v2ce_volume_losses_workspace_bytes(2, 5, 3, 3, hip.VOXLOSSES_TEMPORAL) > 0
    assert L.v2ce_volume_losses_workspace_bytes(2, 10, 8, 8, hip.VOXLOSSES_EF) == 0        # sequence terms need 5-D
    size = ctypes.sizeof(hip.VoxLossesStats)
    assert size == losses.STATS_DTYPE.itemsize == 240
    assert L.v2ce_voxlosses(None, None, 1, 1, 20, 8, 8, every, None, size, None, 0, None) != 0
    assert b"null" in L.v2ce_last_error()
    assert L.v2ce_voxlosses(None, None, 1, 1, 20, 8, 8, every, None, size - 8, None, 0, None) != 0
    assert b"stats_struct_size" in L.v2ce_last_error()
    assert L.v2ce_volume_losses(None, None, 1, 4, 8, 8, hip.VOXLOSSES_TEMPORAL, None, size, None, 0, None) != 0
    assert b"D >= 5" in L.v2ce_last_error()


def test_losses_py_refusals_without_gpu():
    x = torch.zeros(1, 2, 20, 8, 8)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.voxel_losses_batch(x, x)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.calculate_loss(x, x)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.Pyramid3dLoss()(x[0], x[0])
    with pytest.raises(ValueError, match="20"):
        losses.voxel_losses_batch(torch.zeros(1, 2, 18, 8, 8), torch.zeros(1, 2, 18, 8, 8))
    with pytest.raises(ValueError):
        losses.voxel_losses_batch(x[0], x[0])
    with pytest.raises(ValueError, match="contiguous"):
        nc = torch.zeros(1, 2, 20, 8, 16)[..., ::2]
        losses.voxel_losses_batch(nc, nc)
    with pytest.raises(TypeError):
        losses.voxel_losses_batch(x.double(), x.double())
    with pytest.raises(ValueError, match="unknown term"):
        losses.voxel_losses_batch(x, x, terms=("pyramids",))
    for name, why in (("gan", "discriminator"), ("encoder", "VoxelEncoder"), ("imu", "IMU")):
        with pytest.raises(ValueError, match=why):
            losses.calculate_loss(x, x, loss=("pyramid", name))
    with pytest.raises(ValueError, match="unknown loss"):
        losses.calculate_loss(x, x, loss=("pyramyd",))
    with pytest.raises(ValueError, match="ef_type"):
        losses.calculate_loss(x, x, ef_type="c")
    assert losses.terms_for(("pyramid", "pt", "ef_splitp", "physical")) == ("pyramid", "temporal", "ef")
