"""CPU: the float64 restatement of the image-gradient channel (tests/image_grad_ref.py) against the reference's own
results (tests/golden/.imgrad, recipe tests/make_imgrad_goldens.py) within the reference's recorded error; the host's blur
taps; the argument refusals of v2ce_toolbox_amd.image_derivative and of the C entries that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import image_grad_ref as R
from v2ce_toolbox_amd import hip


def load(gold_dir, name):
    return np.load(os.path.join(gold_dir, ".imgrad", f"{name}.npz"))


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_restatement_agrees_with_the_reference_within_its_error(gold_dir, name):
    z = load(gold_dir, name)
    fr, w = z["frames"], z["weights"]
    assert fr.dtype == np.uint8 and fr.ndim == 4 and w.dtype == np.float32 and w.size == int(z["kernel_size"])
    S, L1, H, W = fr.shape
    assert z["blur"].shape == (S, L1 - 1, H, W) and z["units"].shape == (S, L1 - 1, 3, H, W)
    assert z["blur"].dtype == z["units"].dtype == np.float32
    err_blur, err_units = float(z["err_ref_blur"]), float(z["err_ref_units"])
    assert np.isfinite(err_blur) and np.isfinite(err_units) and 0 <= err_blur < 1e-5 and 0 <= err_units < 1e-5
    assert np.abs(R.blurred_gradient(fr, w) - z["blur"]).max() <= err_blur
    c2, gmax = R.units_channel2(fr, w)
    assert np.array_equal(np.isnan(c2), np.isnan(z["units"][:, :, 2]))
    ok = ~np.isnan(c2)
    assert not ok.any() or np.abs(c2[ok] - z["units"][:, :, 2][ok]).max() <= err_units
    assert R.normalised_frames(fr).tobytes() == np.ascontiguousarray(z["units"][:, :, :2]).tobytes()


def test_fixtures_cover_what_they_are_for(gold_dir):
    assert load(gold_dir, "min_6x6")["frames"].shape[-2:] == (6, 6) and int(load(gold_dir, "min_6x6")["kernel_size"]) == 11
    assert load(gold_dir, "ragged_7x70")["frames"].shape[-2:] == (7, 70)
    assert load(gold_dir, "tile_edges")["frames"].shape[-2:] == (R.TILE_H + 1, R.TILE_W + 1)
    hot = load(gold_dir, "one_hot_9x9")["frames"][0]
    assert [np.argwhere(f).tolist() for f in hot] == [[[0, 0]], [[4, 8]], [[4, 4]]] and hot.max() == 255
    k5 = load(gold_dir, "k5_s1p5_21x40")
    assert int(k5["kernel_size"]) == 5 and float(k5["sigma"]) == 1.5
    two = load(gold_dir, "two_packets")
    _, gmax = R.units_channel2(two["frames"], two["weights"])
    assert two["frames"].shape[:2] == (2, 3) and gmax[0] > 20 * gmax[1] > 0           # the maximum is per packet
    assert np.nanmax(two["units"][1, :, 2]) == 1.0 and np.nanmax(two["units"][0, :, 2]) == 1.0
    flat = load(gold_dir, "flat_8x8")
    assert not flat["frames"].any() and not flat["blur"].any() and np.isnan(flat["units"][:, :, 2]).all()
    # zero padding against reflection: a flat bright frame has gradient on its border only
    sq = R.sobel_squares(np.full((5, 5), 200, np.uint8))
    assert sq[1:-1, 1:-1].max() == 0 and sq[0, 0] == 2 * 600 ** 2 and sq[0, 2] == 800 ** 2


def test_the_taps_are_the_goldens_table(gold_dir):
    from v2ce_toolbox_amd import image_derivative as ID
    for name in R.GOLDEN_NAMES:
        z = load(gold_dir, name)
        got = ID.gaussian_taps(int(z["kernel_size"]), float(z["sigma"]))
        assert got.dtype == np.float32 and got.tobytes() == z["weights"].tobytes(), name
    w = ID.gaussian_taps()
    assert w.size == 11 and np.array_equal(w, w[::-1]) and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6
    for bad in (1, 4, 17):
        with pytest.raises(ValueError, match="kernel_size"):
            ID.gaussian_taps(bad)
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            ID.gaussian_taps(11, bad)


def test_argument_refusals_without_gpu():
    from v2ce_toolbox_amd import image_derivative as ID
    fr = np.zeros((3, 1, 12, 13), np.uint8)
    with pytest.raises(ValueError, match="k / 255"):
        ID.get_batch_double_blurred_image_gradient(fr + 0.5, fr + 0.5)
    with pytest.raises(ValueError, match="k / 255"):
        ID.batch_img_gradient(fr.astype(np.float32) + np.float32(2))              # integers as floats: not the / 255 form
    with pytest.raises(ValueError, match="k / 255"):
        ID.image_units_batch(np.full((2, 12, 13), np.nan, np.float32))
    with pytest.raises(ValueError, match="\\[0, 255\\]"):
        ID.batch_img_residual(fr.astype(np.int32) + 256, fr.astype(np.int32))
    with pytest.raises(ValueError, match="b, 1, h, w"):
        ID.get_batch_double_blurred_image_gradient(fr[:, 0], fr[:, 0])
    for bad in (7, [1, 2], np.zeros((0, 1, 12, 13), np.uint8)):                    # a scalar, a list, an empty batch
        with pytest.raises(ValueError, match="b, 1, h, w"):
            ID.get_batch_double_blurred_image_gradient(bad, bad)
        with pytest.raises(ValueError, match="b, c, h, w"):
            ID.batch_img_gradient(bad)
        with pytest.raises(ValueError, match="b, c, h, w"):
            ID.batch_img_residual(bad, bad)
    with pytest.raises(ValueError, match="kernel_size"):
        ID.get_batch_double_blurred_image_gradient(fr, fr, kernel_size=10)
    with pytest.raises(ValueError, match="sigma"):
        ID.get_batch_double_blurred_image_gradient(fr, fr, sigma=0)
    with pytest.raises(ValueError, match="clip"):
        ID.image_units_batch(np.zeros((12, 13), np.uint8))
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        ID.image_units_batch(torch.zeros((3, 12, 13), dtype=torch.uint8))
    with pytest.raises(hip.V2ceHipError, match="no CPU path"):
        ID.batch_img_gradient(fr, device="cpu")


def test_c_entries_refuse_without_touching_the_device():
    L = hip.lib()
    assert L.v2ce_image_grad_workspace_bytes(4, 16, 260, 346) == 4 * 16 * 260 * 346 * 4
    assert L.v2ce_image_grad_workspace_bytes(1, 1, 2, 2) == 16
    for bad in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 1, 8), (1, 1, 8, 1), (1, 1, 0, 8), (-1, 1, 8, 8),
                (1 << 20, 1 << 10, 64, 64)):
        assert L.v2ce_image_grad_workspace_bytes(*bad) == 0, bad
    w = (ctypes.c_float * 15)(*([1 / 15] * 15))
    one = ctypes.c_void_p(16)                          # a non-null address no refused call dereferences

    def grad(S=1, L_=2, H=12, W=13, k=11, frames=one, weights=w, blur=one, gmax=one):
        return L.v2ce_image_grad_batch(frames, S, L_, H, W, weights, k, blur, gmax, None)

    def units(S=1, L_=2, H=12, W=13, k=11, frames=one, weights=w, out=one, gmax=one, ws=one, ws_bytes=1 << 30):
        return L.v2ce_image_units_grad(frames, S, L_, H, W, weights, k, 0.153, 0.165, out, gmax, ws, ws_bytes, None)

    for entry in (grad, units):
        for kw in (dict(k=10), dict(k=1), dict(k=17), dict(k=-3), dict(H=5), dict(W=5), dict(H=0), dict(S=0), dict(L_=0),
                   dict(S=1 << 20, L_=1 << 10, H=64, W=64)):
            assert entry(**kw) == -1, (entry.__name__, kw)
            assert b"kernel_size" in L.v2ce_last_error()
        assert entry(k=11, H=6, W=6, frames=None) == -1 and b"null" in L.v2ce_last_error()
        assert entry(weights=None) == -1 and b"null" in L.v2ce_last_error()
        assert entry(gmax=None) == -1 and b"null" in L.v2ce_last_error()
    assert grad(blur=None) == -1 and b"null" in L.v2ce_last_error()
    assert units(out=None) == -1 and b"null" in L.v2ce_last_error()
    assert units(ws=None) == -1 and b"null" in L.v2ce_last_error()
    assert units(ws_bytes=2 * 12 * 13 * 4 - 1) == -4 and b"workspace" in L.v2ce_last_error()
    assert units(ws=ctypes.c_void_p(18)) == -1 and b"aligned" in L.v2ce_last_error()
