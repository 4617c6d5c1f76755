"""CPU side of the stage-1 loss gradients (v2ce_voxloss_grads / losses.py): the numpy restatement
(tests/voxlossgrads_ref.py) against the reference's own autograd results (tests/golden/.voxlossgrads/), the coefficient
struct of losses.grad_coeffs against its numpy twin, and what the C ABI of include/v2ce_hip_grad.h refuses without a GPU.

Bounds: against the reference's autograd on .double() inputs (ref64_grad) the f64 restatement agrees to 1e-10 of the
largest gradient; rounded to f32 it is no farther from ref64_grad than the reference's own f32 run is (ref32_dev) plus
one f32 rounding of the largest gradient."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import voxlossgrads_ref as G
from tests.make_voxlossgrads_goldens import CONFIGS, FILES, SIZE_CAP, STAGED
from v2ce_toolbox_amd import hip, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".voxlossgrads")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
name_of = lambda p: os.path.basename(p)[:-4]
BAD_ARG, WORKSPACE = -1, -4


def golden_specs(path):
    """(key of the stored gradient, pred, gt, keywords of calculate_loss, stages, index of the stage) per stored gradient."""
    z = np.load(path)
    out = []
    for cfg in FILES[name_of(path)]:
        kw = dict(CONFIGS[cfg])
        if cfg in STAGED:
            out.append((cfg, z, kw, 2, 0))
            out.append((f"{cfg}_p2", z, kw, 2, 1))
        else:
            out.append((cfg, z, kw, 1, 0))
    return out


def test_goldens_are_the_recipes_files_and_small():
    assert [name_of(p) for p in GOLDENS] == sorted(FILES)
    for p in GOLDENS:
        assert os.path.getsize(p) <= SIZE_CAP, p
        z = np.load(p)
        keys = {"pred", "gt"} | ({"pred2"} if any(c in STAGED for c in FILES[name_of(p)]) else set())
        for key, *_ in golden_specs(p):
            keys |= {f"ref64_grad_{key}", f"ref32_dev_{key}"}
        assert set(z.files) == keys, p
        assert z["pred"].dtype == np.float32 and z["gt"].dtype == np.float32
        assert all(z[k].dtype == np.float64 for k in z.files if k.startswith("ref"))
    every = {c for f in FILES.values() for c in f}
    assert every == set(CONFIGS)                                   # each term alone, the lists and the staged run are stored


def test_fixtures_exercise_what_they_are_for():
    z = {name_of(p): np.load(p) for p in GOLDENS}
    assert z["b1_l1_8x8"]["pred"].shape == (1, 1, 20, 8, 8)        # D = 10 = 1 mod 3
    assert z["b2_l3_9x10"]["pred"].shape == (2, 3, 20, 9, 10)      # D = 30 = 0 mod 3, ragged H and W, B > 1
    p = z["at_threshold"]["pred"]
    thr = np.float32(0.01)
    assert (p == thr).sum() > 100 and (p == np.nextafter(thr, np.float32(1))).sum() > 100
    assert not z["zero_gt"]["gt"].any() and not z["zero_pred"]["pred"].any()
    for name, f in z.items():
        if name != "zero_pred":
            assert (f["pred"] == 0).mean() > 0.2, name             # exact zeros: sign(0)
    # the last plane of a volume with D % 3 == 0 is in no 3-window: its 'pt' gradient has no 3-window part
    c = G.coeffs((2, 3, 20, 9, 10), ("pt",))
    t = G.term_grads(z["b2_l3_9x10"]["pred"], z["b2_l3_9x10"]["gt"], c)
    assert not t["t3"][:, 2, [9, 19]].any() and t["t3"][:, 2, [8, 18]].any() and t["t5"][:, 2, [9, 19]].any()
    # elements outside the floored extents get no pyramid gradient
    c = G.coeffs((2, 3, 20, 9, 10), ("pyramid",))
    t = G.term_grads(z["b2_l3_9x10"]["pred"], z["b2_l3_9x10"]["gt"], c)
    assert not t["pyr2"][..., 8, :].any() and not t["pyr4"][..., 8:].any() and not t["pyr8"][:, 2, 4:10].any()
    assert t["pyr2"][..., :8, :].any() and t["pyr4"][:, 2, 4:8, :8, :8].any()


@pytest.mark.parametrize("path", GOLDENS, ids=name_of)
def test_restatement_matches_the_reference_autograd(path):
    for key, z, kw, stages, i in golden_specs(path):
        kw = dict(kw)
        loss = kw.pop("loss")
        got, _ = G.grad(z["pred2"] if i else z["pred"], z["gt"], loss, stages=stages, **kw)
        want = z[f"ref64_grad_{key}"]
        top = np.abs(want).max()
        err = np.abs(got - want).max()
        assert err <= 1e-10 * top, (key, err, top)
        # two-sided: rounded to f32, no farther from the f64 run than the reference's own f32 run, plus one rounding
        err32 = np.abs(got.astype(np.float32).astype(np.float64) - want).max()
        assert err32 <= float(z[f"ref32_dev_{key}"]) + 2.0 ** -23 * top, (key, err32, float(z[f"ref32_dev_{key}"]))


def fields_of(c):
    return {n: (list(getattr(c, n)) if n in ("a_pyr", "a_ef") else getattr(c, n)) for n in G.FIELDS}


@pytest.mark.parametrize("shape", [(2, 3, 20, 11, 13), (1, 1, 20, 8, 8), (3, 16, 20, 260, 346)])
def test_grad_coeffs_equal_their_numpy_twin(shape):
    assert losses.COEFF_FIELDS == G.FIELDS
    opts = [dict(), dict(ef_type="only_c", add_base_loss=True), dict(ef_type="cl", alpha_pyramid=10.0, alpha_ef=2.0),
            dict(alpha_efc=3, alpha_match=0.25, alpha_compensation=4, alpha_norm=1e-3, alpha_pt=7)]
    for loss in [G.DEFAULT_LOSS, G.ALL_LOSS] + [(n,) for n in G.ALL_LOSS] + [("ef", "pt"), ("ef_splitp", "norml2", "l1")]:
        for kw in opts:
            for stages in (1, 2, 3):
                c = losses.grad_coeffs(shape, loss, stages=stages, pred_sq_sum=12.5, **kw)
                assert c.struct_size == ctypes.sizeof(hip.VoxLossGradCoeffs) == 8 * 15
                want = G.coeffs(shape, loss, stages=stages, pred_sq_sum=12.5, **kw)
                assert fields_of(c) == want, (loss, kw, stages)
                one = fields_of(losses.grad_coeffs(shape, loss, stages=1, pred_sq_sum=12.5, **kw))
                for n in G.FIELDS:                                  # / stages, and zero for absent terms
                    assert np.allclose(np.atleast_1d(want[n]) * stages, np.atleast_1d(one[n]), rtol=1e-15, atol=0), n
    c = fields_of(losses.grad_coeffs(shape, ("pyramid",)))
    assert all(c["a_pyr"]) and not any(c[n] for n in G.FIELDS if n != "a_pyr" and not isinstance(c[n], list))
    assert not any(c["a_ef"])
    c = fields_of(losses.grad_coeffs(shape, ("ef",), ef_type="only_c"))
    assert c["a_ef"][0] and not any(c["a_ef"][1:]) and not c["a_sq"]
    assert fields_of(losses.grad_coeffs(shape, ("norml2",), pred_sq_sum=0.0))["a_l2"] == 0.0
    # volumes: the same factors as the sequences they were cut from
    B, Lq, _, H, W = shape
    v = fields_of(losses.grad_coeffs((2 * B, 10 * Lq, H, W), ("pyramid", "pt"), add_base_loss=True))
    assert v == fields_of(losses.grad_coeffs(shape, ("pyramid", "pt"), add_base_loss=True)) == G.coeffs(
        (2 * B, 10 * Lq, H, W), ("pyramid", "pt"), add_base_loss=True)


def test_grad_coeffs_refusals():
    with pytest.raises(ValueError, match="discriminator"):
        losses.grad_coeffs((1, 2, 20, 8, 8), ("pyramid", "gan"))
    with pytest.raises(ValueError, match="smaller than kernel size"):
        losses.grad_coeffs((1, 2, 20, 7, 9), ("pyramid",))
    with pytest.raises(ValueError, match="too small"):
        losses.grad_coeffs((2, 4, 8, 8), ("pt",))
    with pytest.raises(ValueError, match="only"):
        losses.grad_coeffs((2, 10, 8, 8), ("pyramid", "ef"))
    with pytest.raises(ValueError, match="pred_sq_sum"):
        losses.grad_coeffs((1, 2, 20, 8, 8), ("norml2",))
    with pytest.raises(ValueError):
        losses.grad_coeffs((1, 2, 18, 8, 8), ("ef",))
    with pytest.raises(ValueError):
        losses.grad_coeffs((1, 2, 20, 8, 8), ("ef",), ef_type="c")
    with pytest.raises(ValueError):
        losses.grad_coeffs((1, 2, 20, 8, 8), ("ef",), stages=0)


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "v2ce_hip_grad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_grad_header():
    L = hip.lib()
    syms = declared_symbols()
    assert len(syms) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(hip.GRAD_EXPORTS) and len(set(hip.GRAD_EXPORTS)) == len(hip.GRAD_EXPORTS)
    assert not set(hip.GRAD_EXPORTS) & set(hip.EXPORTS)
    main = open(os.path.join(ROOT, "include", "v2ce_hip.h")).read()
    assert not any(s in main for s in syms)


def coef(**kw):
    c = hip.VoxLossGradCoeffs(struct_size=ctypes.sizeof(hip.VoxLossGradCoeffs))
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def test_size_queries_and_null_pointers_without_gpu():
    L = hip.lib()
    size = ctypes.sizeof(hip.VoxLossGradCoeffs)
    seq, vol = L.v2ce_voxloss_grads_workspace_bytes, L.v2ce_volume_loss_grads_workspace_bytes
    full = losses.grad_coeffs((2, 3, 20, 9, 11), G.ALL_LOSS, pred_sq_sum=1.0)
    assert seq(2, 3, 20, 9, 11, ctypes.byref(full), size) > 0
    assert seq(2, 3, 18, 9, 11, ctypes.byref(full), size) == 0                     # C != 20
    assert seq(2, 3, 20, 9, 11, ctypes.byref(full), size - 8) == 0                 # another struct layout
    assert seq(2, 3, 20, 9, 11, ctypes.byref(coef(a_sq=1.0, struct_size=size + 8)), size) == 0
    assert seq(2, 3, 20, 9, 11, None, size) == 0
    assert seq(0, 3, 20, 9, 11, ctypes.byref(full), size) == 0
    assert seq(1, 1, 20, 7, 9, ctypes.byref(coef(a_pyr=[1.0, 1.0, 1.0])), size) == 0           # min(D, H, W) < 8
    assert seq(1, 1, 20, 7, 9, ctypes.byref(coef(a_sq=1.0, a_ef=[1.0, 0, 0, 0])), size) > 0
    v = coef(a_sq=1.0, a_pyr=[1.0, 1.0, 1.0], a_t3=1.0, a_t5=1.0)
    assert vol(2, 25, 9, 10, ctypes.byref(v), size) > 0
    assert vol(2, 7, 9, 10, ctypes.byref(v), size) == 0 and vol(2, 25, 7, 10, ctypes.byref(v), size) == 0
    assert vol(2, 4, 9, 10, ctypes.byref(coef(a_t3=1.0)), size) == 0 and vol(2, 4, 9, 10, ctypes.byref(coef(a_t5=1.0)), size) == 0
    assert vol(2, 5, 3, 3, ctypes.byref(coef(a_t3=1.0, a_t5=1.0)), size) > 0       # temporal needs D >= 5 only
    assert vol(2, 4, 9, 10, ctypes.byref(coef(a_sq=1.0)), size) > 0
    for k in ("a_comp", "a_match", "a_l1", "a_l2"):                                # non-volume factors on the volume entry
        assert vol(2, 25, 9, 10, ctypes.byref(coef(a_sq=1.0, **{k: 1.0})), size) == 0, k
    assert vol(2, 25, 9, 10, ctypes.byref(coef(a_ef=[0, 0, 1.0, 0])), size) == 0
    assert vol(2, 25, 9, 10, ctypes.byref(v), size - 8) == 0
    # null pointers: refused before anything is launched
    assert L.v2ce_voxloss_grads(None, None, 2, 3, 20, 9, 11, ctypes.byref(full), size, None, None, None, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    assert L.v2ce_volume_loss_grads(None, None, 2, 25, 9, 10, ctypes.byref(v), size, None, None, None, 0, None) == BAD_ARG
    assert b"null" in L.v2ce_last_error()
    assert L.v2ce_voxloss_grads(None, None, 2, 3, 20, 9, 11, None, size, None, None, None, 0, None) == BAD_ARG
    assert L.v2ce_voxloss_grads(None, None, 2, 3, 18, 9, 11, ctypes.byref(full), size, None, None, None, 0, None) == BAD_ARG
    assert b"20 channels" in L.v2ce_last_error()
    assert L.v2ce_volume_loss_grads(None, None, 2, 25, 9, 10, ctypes.byref(v), size - 8, None, None, None, 0, None) == BAD_ARG
    assert b"struct_size" in L.v2ce_last_error()


def test_python_refusals_without_gpu():
    x = torch.zeros(1, 2, 20, 8, 8)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.voxel_loss_grads_batch(x, x)
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.volume_loss_grads_batch(x[0], x[0])
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        losses.calculate_loss(x.clone().requires_grad_(), x)
    with pytest.raises(ValueError, match="float32"):
        losses.voxel_loss_grads_batch(x.double(), x.double())
    with pytest.raises(ValueError, match="contiguous"):
        losses.voxel_loss_grads_batch(torch.zeros(1, 2, 20, 8, 16)[..., ::2], x)
    with pytest.raises(ValueError):
        losses.voxel_loss_grads_batch(x[0], x[0])
