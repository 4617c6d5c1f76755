"""GPU: the device event-frame video (csrc/event_frames.hip through the C ABI; event_frames.EventFrameRenderer) against
the host path it replaces (pipeline.event_frame_sums + v2ce.event_frame_images), numpy's integer counts and the
reference's own frames (golden G9, tests/golden/.efvideo/).  Equality is equality of bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import event_frames_ref as R
from tests.test_event_frames_cpu import all_cases, same_scalar
from v2ce_toolbox_amd import event_frames as EF
from v2ce_toolbox_amd import glue, hip, pipeline, synth, v2ce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gamma_vox(rng, shape, density=0.4):
    return (rng.gamma(0.3, 1.2, shape) * (rng.random(shape) < density)).astype(np.float32)


def renderer_for(vox, keep, ceil=10, q=98):
    return EF.EventFrameRenderer(keep, ceil, q, vox.shape[3], vox.shape[4], "cuda")


def host_upper(S, ceil, q, keep):
    efs = np.concatenate([S[:, :2], np.zeros_like(S[:, :1], dtype=np.float64)], 1) if keep else np.repeat(S[:, 2:3], 3, 1)
    return min(np.percentile(efs[efs > 0], q), ceil)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 9, 14), (5, 11, 13), (2, 3, 400), (4, 8, 12), (64, 260, 346)])
def test_fused_sums_equal_event_frame_sums(shape):
    P, H, W = shape
    rng = np.random.default_rng(P * 1000 + H)
    vox = dev(gamma_vox(rng, (P, 2, 10, H, W)))
    want = pipeline.event_frame_sums(vox)
    for keep in (True, False):
        got = EF.EventFrameRenderer(keep, 10, 98, H, W, "cuda").add(0, vox)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), keep
    if H * W % 4 == 0:                                           # the same through the scalar path: a 4-B aligned base
        big = torch.zeros(1 + vox.numel(), device="cuda")
        mis = big[1:].view(vox.shape)
        mis.copy_(vox)
        got = EF.EventFrameRenderer(True, 10, 98, H, W, "cuda").add(0, mis)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def add_in_batches(r, vox, cuts, reverse=False):
    parts = [(a, vox[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for a, v in (reversed(parts) if reverse else parts):
        r.add(a, v.contiguous())


@pytest.mark.parametrize("keep", [True, False])
def test_histograms_equal_numpy_and_do_not_depend_on_batching(keep):
    rng = np.random.default_rng(7)
    L, H, W = 23, 17, 22
    vox_h = gamma_vox(rng, (L, 2, 10, H, W))
    vox_h[3:6] = np.round(vox_h[3:6] * 2) / 2                     # ties
    vox = dev(vox_h)
    bits = R.positive_bits(R.sums(vox_h), keep)
    s = np.sort(bits)
    ra, rb = int(bits.size * 0.37), int(bits.size * 0.98)
    pa, pb = int(s[ra] >> 20), int(s[rb] >> 20)
    seen = []
    for cuts, rev in (([0, L], False), ([0, 2, 3, 9, 10, 15, 22, L], False), ([0, 2, 3, 9, 10, 15, 22, L], True), ([0, L], False)):
        r = renderer_for(vox_h, keep)
        add_in_batches(r, vox, cuts, rev)
        h0 = r.level0_histogram()
        h1 = r.refine_histogram(1, pa, pb)
        h2 = r.refine_histogram(2, int(s[ra] >> 10), int(s[rb] >> 10))
        assert np.array_equal(h0, R.level0_hist(bits))
        assert np.array_equal(h1, np.stack([R.refine_hist(bits, 1, pa), R.refine_hist(bits, 1, pb)]))
        assert np.array_equal(h2, np.stack([R.refine_hist(bits, 2, int(s[ra] >> 10)), R.refine_hist(bits, 2, int(s[rb] >> 10))]))
        a, b = r.order_statistics(ra, rb)
        assert a.view(np.uint32) == s[ra] and b.view(np.uint32) == s[rb]
        seen.append((h0.tobytes(), h1.tobytes(), h2.tobytes()))
    assert len(set(seen)) == 1
    # additive state: two partial histograms summed == the histogram of the union
    r1, r2 = renderer_for(vox_h, keep), renderer_for(vox_h, keep)
    r1.add(0, vox[:9].contiguous())
    r2.add(9, vox[9:].contiguous())
    assert np.array_equal(r1.level0_histogram() + r2.level0_histogram(), R.level0_hist(bits))
    r1.reset()
    assert r1.level0_histogram().sum() == 0


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("ceil", [1, 1000])
@pytest.mark.parametrize("q", [0, 50, 90, 98, 100])
def test_frames_and_upper_equal_the_host(keep, ceil, q):
    rng = np.random.default_rng(11)
    L, H, W = 9, 13, 19
    vox_h = gamma_vox(rng, (L, 2, 10, H, W))
    S = pipeline.event_frame_sums(torch.from_numpy(vox_h)).numpy()
    r = renderer_for(vox_h, keep, ceil, q)
    add_in_batches(r, dev(vox_h), [0, 4, 5, L], reverse=True)
    frames, upper = r.finish()
    want_upper = host_upper(S, ceil, q, keep)
    assert same_scalar(upper, want_upper), (upper, want_upper)
    bits = np.sort(R.positive_bits(S, keep))
    mult = 1 if keep else 3
    assert r.last["n"] == bits.size * mult
    for rank, val in zip(r.last["ranks"], r.last["order_stats"]):
        assert val.view(np.uint32) == bits[rank // mult]
    assert frames.dtype == np.uint8 and frames.shape == (L, H, W, 3)
    assert frames.tobytes() == v2ce.event_frame_images(S, ceil, q, keep).tobytes()


@pytest.mark.parametrize("case", [c[0] for c in all_cases()])
def test_frames_equal_the_reference_fixtures(case):
    _, vox, runs = next(c for c in all_cases() if c[0] == case)
    for name, keep, ceil, pct, want in runs:
        r = renderer_for(vox, keep, ceil, pct)
        cuts = sorted({0, vox.shape[0] // 2, vox.shape[0]})
        add_in_batches(r, dev(vox), cuts)
        frames, upper = r.finish()
        assert frames.tobytes() == np.ascontiguousarray(want).tobytes(), (case, name)
        assert same_scalar(upper, host_upper(R.sums(vox), ceil, pct, keep)), (case, name)


def test_no_positive_value_raises_like_the_host():
    r = EF.EventFrameRenderer(True, 10, 98, 6, 8, "cuda")
    r.add(0, torch.zeros(2, 2, 10, 6, 8, device="cuda"))
    with pytest.raises(IndexError):
        r.finish()


@pytest.mark.parametrize("kind", ["relu_randn", "gamma"])
def test_full_size_two_batches(kind):
    """Two 64-pair batches at 260x346, both modes, against the host path on the same sums."""
    if kind == "relu_randn":
        vox_h = synth.synthetic_voxels(128, 260, 346, seed=3, regime="sparse")
    else:
        rng = np.random.default_rng(13)
        vox_h = rng.standard_gamma(0.3, (128, 2, 10, 260, 346), dtype=np.float32) * np.float32(1.2)
    vox = dev(vox_h)
    S = torch.cat([pipeline.event_frame_sums(vox[:64]), pipeline.event_frame_sums(vox[64:])]).cpu().numpy()
    del vox_h
    for keep in (True, False):
        r = EF.EventFrameRenderer(keep, 10, 98, 260, 346, "cuda")
        s1 = r.add(64, vox[64:])
        s0 = r.add(0, vox[:64])
        assert torch.cat([s0, s1]).cpu().numpy().tobytes() == S.tobytes()
        frames, upper = r.finish()
        assert same_scalar(upper, host_upper(S, 10, 98, keep))
        assert frames.tobytes() == v2ce.event_frame_images(S, 10, 98, keep).tobytes(), keep


@pytest.mark.parametrize("infer_type,wf", [("center", 48), ("pano", 112)])
@pytest.mark.parametrize("keep", ["true", "false"])
def test_cli_writes_the_host_paths_frames(tmp_path, infer_type, wf, keep):
    """python v2ce.py --write_event_frame_video true: the written frames == event_frame_images of event_frame_sums of the
    same run's voxels (the model is deterministic: the voxels are rebuilt here with the same weights and frames)."""
    try:
        import cv2  # noqa: F401
        pytest.skip("with OpenCV the frames go into an mp4")
    except ImportError:
        pass
    out = tmp_path / "out"
    frames_path = tmp_path / "frames.npy"
    fr = synth.synthetic_frames(37, 32, wf, seed=9)
    np.save(frames_path, fr)
    cmd = [sys.executable, os.path.join(ROOT, "v2ce.py"), "--npy_frames", str(frames_path), "--height", "32", "--width", "48",
           "--synthetic_weights", "0", "-o", str(out), "-b", "2", "--seed", "11", "-t", infer_type,
           "--write_event_frame_video", "true", "--vis_keep_polarity", keep, "--max_frame_num", "37"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    color = "rgb" if keep == "true" else "gray"
    path = out / f"{infer_type}-frames-ceil_10-fps_30-pred_ef_{color}.npz"
    assert path.exists(), os.listdir(out)
    from v2ce_toolbox_amd.v2ce_3d import V2ce3d
    m = V2ce3d()
    m.load_state_dict(synth.make_state_dict(0))
    vox = glue.video_to_voxels(m.eval().to("cuda"), frames=fr, infer_type=infer_type, width=48, height=32, batch_size=2)
    want = v2ce.event_frame_images(pipeline.event_frame_sums(vox).cpu().numpy(), 10, 98, keep == "true")
    assert np.load(path)["event_frames"].tobytes() == want.tobytes()
    # and the host path behind its switch writes the same file
    env = dict(os.environ, V2CE_EVENT_FRAMES="host")
    out2 = tmp_path / "out2"
    cmd[cmd.index(str(out))] = str(out2)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.load(out2 / path.name)["event_frames"].tobytes() == want.tobytes()
