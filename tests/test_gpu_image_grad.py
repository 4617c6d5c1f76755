"""GPU: the image-gradient channel and the three-channel image units (v2ce_image_grad_batch, v2ce_image_units_grad through
v2ce_toolbox_amd.image_derivative) against the float64 truth of tests/image_grad_ref.py and the reference's recorded
results (tests/golden/.imgrad).

The reference's channel 2 is the outcome of two float32 convolutions, so its bytes are no contract.  The conditions:
  * blur:     max |kernel - truth| <= max(1.25 * err_ref_blur, one float32 ulp at the packet's maximum), err_ref_blur the
              reference's own error against the same truth (recorded in the golden);
  * channel 2 of the units: the same with err_ref_units and the ulp at 1.0, the normalised packet maximum;
  * |kernel - reference| <= err_ref + err_kernel (the triangle inequality; err_kernel as measured in the same test);
  * channels 0 / 1: the bytes of the reference's frame_normalize and of v2ce_preprocess_pairs;
  * every output bit-identical run to run, and a packet's outputs bit-identical alone and inside a larger call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_grad_ref as R
from v2ce_toolbox_amd import glue, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(gold_dir, name):
    return np.load(os.path.join(gold_dir, ".imgrad", f"{name}.npz"))


def same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first in cell "
                           f"{np.unravel_index(bad[0] // want.itemsize, want.shape)}: "
                           f"{got.reshape(-1)[bad[0] // want.itemsize]!r} != {want.reshape(-1)[bad[0] // want.itemsize]!r}")


def max_err(got, truth):
    """Largest |got - truth| over the cells where the truth is a number; NaN must sit where the truth has it."""
    assert np.array_equal(np.isnan(got), np.isnan(truth))
    ok = ~np.isnan(truth)
    return float(np.abs(got[ok].astype(np.float64) - truth[ok]).max()) if ok.any() else 0.0


def check_against_truth(frames, taps, blur, units, gmax, err_ref_blur, err_ref_units, what, ref_blur=None, ref_units=None):
    """The conditions of the module docstring for one call's outputs (host arrays)."""
    truth = R.blurred_gradient(frames, taps)
    truth_c2, truth_max = R.units_channel2(frames, taps)
    same_bytes(gmax, blur.reshape(blur.shape[0], -1).max(axis=1), f"{what}: gmax is the packet's largest blur value")
    same_bytes(units[:, :, :2], R.normalised_frames(frames), f"{what}: channels 0 / 1")
    for s in range(frames.shape[0]):
        err_b = max_err(blur[s], truth[s])
        err_u = max_err(units[s, :, 2], truth_c2[s])
        bound_b = max(1.25 * err_ref_blur, R.ulp32(truth_max[s]))
        bound_u = max(1.25 * err_ref_units, R.ulp32(1.0))
        print(f"{what} packet {s}: blur err {err_b:.3e} (bound {bound_b:.3e}, reference {err_ref_blur:.3e}), "
              f"units err {err_u:.3e} (bound {bound_u:.3e}, reference {err_ref_units:.3e})")
        assert err_b <= bound_b, (what, s, err_b, bound_b)
        assert err_u <= bound_u, (what, s, err_u, bound_u)
        if ref_blur is not None:
            assert max_err(blur[s], ref_blur[s].astype(np.float64)) <= err_ref_blur + err_b, (what, s)
            assert max_err(units[s, :, 2], ref_units[s, :, 2].astype(np.float64)) <= err_ref_units + err_u, (what, s)
            same_bytes(units[s, :, :2], ref_units[s, :, :2], f"{what}: the reference's frame_normalize")


@pytest.mark.parametrize("name", R.GOLDEN_NAMES)
def test_goldens(gold_dir, name):
    from v2ce_toolbox_amd import image_derivative as ID
    z = load(gold_dir, name)
    frames, k, sigma = z["frames"], int(z["kernel_size"]), float(z["sigma"])
    S, L1, H, W = frames.shape
    dev = torch.from_numpy(frames).cuda()
    units, gmax = ID.image_units_batch(dev, sigma=sigma, kernel_size=k)
    assert units.shape == (S, L1 - 1, 3, H, W) and gmax.shape == (S,) and units.dtype == gmax.dtype == torch.float32
    blur = torch.stack([ID.get_batch_double_blurred_image_gradient(dev[s, :-1, None], dev[s, 1:, None], sigma, k)[:, 0]
                        for s in range(S)])
    u, g, b = units.cpu().numpy(), gmax.cpu().numpy(), blur.cpu().numpy()
    check_against_truth(frames, z["weights"], b, u, g, float(z["err_ref_blur"]), float(z["err_ref_units"]), name,
                        z["blur"], z["units"])
    if name == "flat_8x8":
        assert g.tolist() == [0.0] and np.isnan(u[:, :, 2]).all() and not b.any()
    # channels 0 / 1 are v2ce_preprocess_pairs' bytes
    for s in range(S):
        same_bytes(units[s, :, :2], glue.image_pre_processing_device(dev[s]), "v2ce_preprocess_pairs")
    # run to run
    units2, gmax2 = ID.image_units_batch(dev, sigma=sigma, kernel_size=k)
    same_bytes(units2, u, "second run")
    same_bytes(gmax2, g, "second run, gmax")
    # a packet alone and inside a larger call (next to brighter, mirrored and darker packets)
    other = np.stack([255 - frames[0, :, ::-1], frames[0, :, :, ::-1] // 3])
    big = torch.from_numpy(np.concatenate([other[:1], frames, other[1:]])).cuda()
    ub, gb = ID.image_units_batch(big, sigma=sigma, kernel_size=k)
    same_bytes(ub[1:1 + S], u, "inside a larger call")
    same_bytes(gb[1:1 + S], g, "inside a larger call, gmax")
    for s in range(S):
        us, gs = ID.image_units_batch(dev[s], sigma=sigma, kernel_size=k)           # a clip [L+1, H, W]
        same_bytes(us[0], u[s], "alone")
        same_bytes(gs, g[s:s + 1], "alone, gmax")


def test_drop_ins_take_uint8_and_k255_floats_only(gold_dir):
    from v2ce_toolbox_amd import image_derivative as ID
    z = load(gold_dir, "r37x50")
    fr = z["frames"][0]                                                # [5, 37, 50]
    a, b = fr[:-1, None], fr[1:, None]
    want = ID.get_batch_double_blurred_image_gradient(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert want.shape == (4, 1, 37, 50) and want.dtype == torch.float32 and want.is_cuda
    truth = R.blurred_gradient(fr[None], z["weights"])[0]
    assert max_err(want[:, 0].cpu().numpy(), truth) <= 1.25 * float(z["err_ref_blur"])
    fa, fb = torch.from_numpy(a).float() / 255, torch.from_numpy(b).float() / 255         # the reference's own input
    same_bytes(ID.get_batch_double_blurred_image_gradient(fa.cuda(), fb.cuda()), want, "k / 255 device floats")
    same_bytes(ID.get_batch_double_blurred_image_gradient(fa.numpy(), fb.numpy()), want, "k / 255 host floats")
    same_bytes(ID.get_batch_double_blurred_image_gradient(a, b), want, "uint8 host arrays")
    same_bytes(ID.get_batch_double_blurred_image_gradient(a.astype(np.float64) / 255, b.astype(np.float64) / 255), want,
               "k / 255 float64")
    for bad in (torch.full((1, 1, 8, 8), 0.5).cuda(), fa.cuda() * 255, fa.cuda() + 1e-4, np.full((1, 1, 8, 8), 0.5, np.float32)):
        with pytest.raises(ValueError, match="k / 255"):
            ID.get_batch_double_blurred_image_gradient(bad, bad)
        with pytest.raises(ValueError, match="k / 255"):
            ID.batch_img_gradient(bad)
        with pytest.raises(ValueError, match="k / 255"):
            ID.batch_img_residual(bad, bad)
    with pytest.raises(ValueError, match="smaller than"):
        ID.get_batch_double_blurred_image_gradient(a[..., :5], b[..., :5])            # W = 5 < 11 // 2 + 1
    with pytest.raises(ValueError, match="smaller than"):
        ID.image_units_batch(fr[:, :5])
    # the gradient and the residual are float32 by definition: correctly rounded sqrt and division, one subtraction
    sq = R.sobel_squares(fr).astype(np.float32)
    grad = np.sqrt(sq) / np.float32(255)
    same_bytes(ID.batch_img_gradient(fa.cuda()), grad[:-1, None], "batch_img_gradient")
    same_bytes(ID.batch_img_gradient(fr[None]), grad[None], "batch_img_gradient, c = 5")
    x = fr.astype(np.float32) / np.float32(255)
    same_bytes(ID.batch_img_residual(fa.cuda(), fb.cuda()), (x[1:] - x[:-1])[:, None], "batch_img_residual")
    same_bytes(ID.batch_img_residual(fr[None, :3], fr[None, 2:]), (x[2:] - x[:3])[None], "batch_img_residual, c = 3")


def test_full_size_packet(gold_dir):
    """One packet of the recording's size (16 pairs of 260 x 346: 5 x 6 tiles of 16 x 64 and ragged ones on both sides)
    against the truth computed here; the bound is formed from the reference's error on r37x50."""
    from v2ce_toolbox_amd import image_derivative as ID
    z = load(gold_dir, "r37x50")
    frames = synth.synthetic_frames(17, 260, 346, seed=5)[None]
    assert frames.dtype == np.uint8 and frames.shape == (1, 17, 260, 346)
    dev = torch.from_numpy(frames).cuda()
    units, gmax = ID.image_units_batch(dev)
    blur = ID.get_batch_double_blurred_image_gradient(dev[0, :-1, None], dev[0, 1:, None])[None, :, 0]
    check_against_truth(frames, ID.gaussian_taps(), blur.cpu().numpy(), units.cpu().numpy(), gmax.cpu().numpy(),
                        float(z["err_ref_blur"]), float(z["err_ref_units"]), "full size")
    again, gmax2 = ID.image_units_batch(dev)
    same_bytes(again, units, "second run")
    same_bytes(gmax2, gmax, "second run, gmax")


def test_two_channel_units_and_packets_of_a_clip():
    from v2ce_toolbox_amd import image_derivative as ID
    clip = synth.synthetic_frames(9, 21, 40, seed=2)
    dev = torch.from_numpy(clip).cuda()
    pairs = glue.image_pre_processing_device(dev)                                        # [8, 2, 21, 40]
    u2, none = ID.image_units_batch(dev, apply_image_grad=False)
    assert none is None
    same_bytes(u2, pairs[None], "two channels, one packet")
    u2, _ = ID.image_units_batch(dev, seq_len=4, apply_image_grad=False)
    same_bytes(u2, pairs.reshape(2, 4, 2, 21, 40), "two channels, packets of 4")
    u3, g3 = ID.image_units_batch(dev, seq_len=4)
    assert u3.shape == (2, 4, 3, 21, 40) and g3.shape == (2,)
    same_bytes(u3[:, :, :2], u2, "three channels, packets of 4")
    for s in range(2):
        us, gs = ID.image_units_batch(dev[4 * s:4 * s + 5])
        same_bytes(us[0], u3[s], "packet of a clip")
        same_bytes(gs, g3[s:s + 1], "packet of a clip, gmax")
    with pytest.raises(ValueError, match="does not split"):
        ID.image_units_batch(dev, seq_len=3)
    cu, cg = ID.clip_image_units(dev, seq_len=3)                                        # 3 + 3 + 2 pairs
    assert cu.shape == (8, 3, 21, 40) and cg.shape == (3,)
    us, gs = ID.image_units_batch(dev[6:])
    same_bytes(cu[6:], us[0], "the short last packet")
    same_bytes(cg[2:], gs, "the short last packet, gmax")


def test_command_line_writes_what_the_api_returns(tmp_path):
    from v2ce_toolbox_amd import image_derivative as ID
    clip = synth.synthetic_frames(5, 21, 40, seed=4)
    rng = np.random.default_rng(3)
    ev = np.zeros(60, np.dtype([("timestamp", "<i8"), ("x", "<i2"), ("y", "<i2"), ("polarity", "i1")]))
    ev["timestamp"] = np.sort(rng.integers(0, 133333, 60))
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, 40, 60), rng.integers(0, 21, 60), rng.choice([-1, 1], 60)
    np.save(tmp_path / "clip.npy", clip)
    np.savez(tmp_path / "events.npz", event_stream=ev)
    base = [sys.executable, os.path.join(ROOT, "v2ce_prep.py"), "--frames", str(tmp_path / "clip.npy"), "--events",
            str(tmp_path / "events.npz"), "--fps", "30", "-l", "error"]
    run = subprocess.run(base + ["--image_grad", "-o", str(tmp_path / "grad")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "grad")) == ["image_grad_max.npy", "image_units.npy", "lfr.npy", "physical_att.npy",
                                                     "status.npy"]
    units, gmax = ID.image_units_batch(clip)
    assert units.shape == (1, 4, 3, 21, 40)
    same_bytes(np.load(tmp_path / "grad" / "image_units.npy"), units[0], "image_units.npy")
    same_bytes(np.load(tmp_path / "grad" / "image_grad_max.npy"), gmax, "image_grad_max.npy")
    # pieces of whole packets: packets of 3 + 1 pairs, one packet per device call
    run = subprocess.run(base + ["--image_grad", "--seq_len", "3", "--chunk", "3", "-o", str(tmp_path / "pieces")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    units, gmax = ID.clip_image_units(clip, seq_len=3)
    assert units.shape == (4, 3, 21, 40) and gmax.shape == (2,)
    same_bytes(np.load(tmp_path / "pieces" / "image_units.npy"), units, "image_units.npy in pieces")
    same_bytes(np.load(tmp_path / "pieces" / "image_grad_max.npy"), gmax, "image_grad_max.npy in pieces")
    run = subprocess.run(base + ["-o", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "plain")) == ["lfr.npy", "physical_att.npy", "status.npy"]
    for name in ("lfr.npy", "physical_att.npy", "status.npy"):
        same_bytes(np.load(tmp_path / "plain" / name), np.load(tmp_path / "grad" / name), name)
