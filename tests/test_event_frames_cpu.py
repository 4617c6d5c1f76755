"""CPU side of the device event-frame video (event_frames.py, csrc/event_frames.hip): np.percentile restated on two
order statistics, the numpy restatement of the three-level selection and of the renderer (tests/event_frames_ref.py)
against np.sort, the host's event_frame_images and the reference's own frames (golden G9 and tests/golden/.efvideo/),
the fixture recipe, the C ABI's refusals and the missing CPU path.  Equality is equality of bytes."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import event_frames_ref as R
from v2ce_toolbox_amd import event_frames as EF
from v2ce_toolbox_amd import hip, v2ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".efvideo")
G9 = os.path.join(ROOT, "tests", "golden", "event_frames_g9.npz")
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "efvideo_*.npz")))


def golden_runs(path):
    """(vox, [(name, keep_polarity, ceil, percentile, rgb frames)]) of one fixture file."""
    z = np.load(path)
    runs = []
    for k in z.files:
        if k.startswith("args_"):
            keep, ceil, pct = (int(v) for v in z[k])
            runs.append((k[5:], bool(keep), ceil, pct, z["bgr_" + k[5:]][..., ::-1]))
    return z["vox"], runs


def same_scalar(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_percentile(x, mult, dtype, q):
    arr = np.repeat(x, mult).astype(dtype)
    want = np.percentile(arr, q)
    s = np.sort(x)
    got = EF.percentile_from_order_stats(len(arr), q, lambda i: s[i // mult], dtype)
    assert same_scalar(want, got), (dtype.__name__, len(arr), q, want, got)
    prev, nxt = EF.percentile_ranks(len(arr), q, dtype)
    assert 0 <= prev <= nxt <= len(arr) - 1 and nxt - prev <= 1


@pytest.mark.parametrize("dtype,mult", [(np.float32, 3), (np.float64, 1)])
def test_percentile_from_order_stats_small_n_every_q(dtype, mult):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 7):
        x = rng.gamma(0.3, 1.2, n).astype(np.float32)
        for q in range(101):
            check_percentile(x, mult, dtype, q)


@pytest.mark.parametrize("dtype,mult", [(np.float32, 3), (np.float64, 1)])
def test_percentile_from_order_stats_random(dtype, mult):
    rng = np.random.default_rng(2)
    for _ in range(1500):
        n, q = int(rng.integers(1, 400)), int(rng.integers(0, 101))
        x = rng.gamma(0.3, 1.2, n).astype(np.float32)
        if n % 5 == 0:
            x = np.round(x * 2) / 2 + np.float32(0.5)            # ties
        check_percentile(x, mult, dtype, q)


@pytest.mark.slow
def test_percentile_from_order_stats_beyond_2_24_float32():
    """3 x 5 592 406 = 16 777 218 float32 values: the float32 virtual index is coarse there; that is part of the contract."""
    rng = np.random.default_rng(3)
    x = rng.gamma(0.3, 1.2, 5_592_406).astype(np.float32)
    for q in (98, 90, 50, 1, 100):
        check_percentile(x, 3, np.float32, q)


def test_goldens_present():
    assert len(GOLDENS) == 6
    for p in GOLDENS:
        assert os.path.getsize(p) <= 300 * 1024, p


def all_cases():
    z = np.load(G9)
    yield "g9", z["vox"], [(n, bool(z[f"args_{n}"][0]), int(z[f"args_{n}"][1]), int(z[f"args_{n}"][2]), z[f"bgr_{n}"][..., ::-1])
                           for n in ("rgb", "gray", "rgb_ceil")]
    for p in GOLDENS:
        vox, runs = golden_runs(p)
        yield os.path.basename(p)[8:-4], vox, runs


def test_selection_matches_sort():
    rng = np.random.default_rng(4)
    for name, vox, _ in all_cases():
        S = R.sums(vox)
        for keep in (True, False):
            bits = R.positive_bits(S, keep)
            s = np.sort(bits)
            assert int(R.level0_hist(bits).sum()) == bits.size
            for r in {0, bits.size // 2, bits.size - 1, *rng.integers(0, bits.size, 5).tolist()}:
                got = R.select(bits.copy(), int(r))
                assert got.dtype == np.float32 and got.view(np.uint32) == s[r], (name, keep, r)


def test_two_bins_fixture_really_splits_the_ranks():
    vox, _ = golden_runs(os.path.join(GOLD, "efvideo_two_bins.npz"))
    bits = np.sort(R.positive_bits(R.sums(vox), True))
    prev, nxt = EF.percentile_ranks(bits.size, 50, np.float64)
    assert nxt == prev + 1 and bits[prev] >> 20 != bits[nxt] >> 20


@pytest.mark.parametrize("case", [c[0] for c in all_cases()])
def test_restatement_matches_reference_and_host(case):
    """The scheme the device follows == the reference's frames == the host's event_frame_images, upper included."""
    _, vox, runs = next(c for c in all_cases() if c[0] == case)
    S = R.sums(vox)
    assert S.tobytes() == __import__("v2ce_toolbox_amd.pipeline", fromlist=["x"]).event_frame_sums(torch.from_numpy(vox)).numpy().tobytes()
    for name, keep, ceil, pct, want in runs:
        got, upper = R.frames(S, ceil, pct, keep, EF.percentile_from_order_stats)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (case, name)
        assert got.tobytes() == v2ce.event_frame_images(S, ceil, pct, keep).tobytes(), (case, name)
        efs = np.concatenate([S[:, :2], np.zeros_like(S[:, :1], dtype=np.float64)], 1) if keep else np.repeat(S[:, 2:3], 3, 1)
        assert same_scalar(upper, min(np.percentile(efs[efs > 0], pct), ceil)), (case, name)


def test_restatement_matches_host_on_random_clips():
    rng = np.random.default_rng(5)
    for trial in range(60):
        L, H, W = int(rng.integers(1, 5)), int(rng.integers(1, 12)), int(rng.integers(1, 15))
        shape = (L, 2, 10, H, W)
        vox = (rng.gamma(0.3, 1.2, shape) * (rng.random(shape) < rng.random())).astype(np.float32)
        if trial % 7 == 0:
            vox = (np.round(vox * 2) / 2).astype(np.float32)
        if trial % 11 == 0:
            vox = vox * np.float32(1e-40)
        S = R.sums(vox)
        if not (S[:, :2] > 0).any():
            continue
        for keep in (True, False):
            for ceil, pct in ((10, 98), (2, 90), (1, 100), (10, 0), (10, 50)):
                got, _ = R.frames(S, ceil, pct, keep, EF.percentile_from_order_stats)
                assert got.tobytes() == v2ce.event_frame_images(S, ceil, pct, keep).tobytes(), (trial, keep, ceil, pct)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "v2ce.py")), reason="the reference tree is not on this machine")
def test_recipe_regenerates_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "make_efvideo_goldens.py"), str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    made = sorted(os.listdir(tmp_path))
    assert made == sorted(os.path.basename(p) for p in GOLDENS)
    for f in made:
        a, b = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(GOLD, f))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (f, k)


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    L = hip.lib()
    assert L.v2ce_event_frames_hist_bytes(0) == 8 * hip.EVENT_FRAMES_LEVEL0_BINS
    assert L.v2ce_event_frames_hist_bytes(1) == L.v2ce_event_frames_hist_bytes(2) == 16 * hip.EVENT_FRAMES_REFINE_BINS
    assert L.v2ce_event_frames_hist_bytes(3) == 0 and L.v2ce_event_frames_hist_bytes(-1) == 0
    assert L.v2ce_event_frames_sums(None, 1, 4, 4, 0, None, None, None) == -1 and b"null" in L.v2ce_last_error()
    for P, H, W, mode in [(0, 4, 4, 0), (1, 0, 4, 0), (1, 4, -1, 1), (1, 4, 4, 2), (1, 4, 4, -1)]:
        assert L.v2ce_event_frames_sums(16, P, H, W, mode, 16, 16, None) == -1, (P, H, W, mode)
    assert L.v2ce_event_frames_sums(16, 1 << 20, 1 << 10, 1 << 10, 0, 16, 16, None) == -2
    assert L.v2ce_event_frames_sums(16, 1, 1 << 14, 1 << 14, 0, 16, 16, None) == -2
    assert L.v2ce_event_frames_refine(16, 1, 4, 4, 0, 3, 0, 0, 16, None) == -1 and b"level" in L.v2ce_last_error()
    assert L.v2ce_event_frames_refine(16, 1, 4, 4, 0, 1, 2048, 0, 16, None) == -1
    assert L.v2ce_event_frames_refine(16, 1, 4, 4, 1, 2, 0, 1 << 21, 16, None) == -1
    assert L.v2ce_event_frames_refine(16, 1, 4, 4, 1, 2, 0, 0, None, None) == -1 and b"null" in L.v2ce_last_error()
    for upper in (0.0, -1.0, float("nan"), float("inf")):
        assert L.v2ce_event_frames_render(16, 1, 4, 4, 0, upper, 0, 1, 16, None) == -1 and b"upper" in L.v2ce_last_error()
    assert L.v2ce_event_frames_render(16, 1, 4, 4, 1, 1e-60, 0, 1, 16, None) == -1          # zero in float32
    assert L.v2ce_event_frames_render(16, 2, 4, 4, 0, 1.0, 3, 4, 16, None) == -1 and b"outside" in L.v2ce_last_error()
    assert L.v2ce_event_frames_render(16, 1, 4, 4, 0, 1.0, -1, 4, 16, None) == -1
    assert L.v2ce_event_frames_render(16, 1, 4, 4, 0, 1.0, 0, 1, 18, None) == -1 and b"aligned" in L.v2ce_last_error()
    assert L.v2ce_event_frames_render(None, 1, 4, 4, 0, 1.0, 0, 1, 16, None) == -1


def test_no_cpu_path():
    with pytest.raises(hip.V2ceHipError):
        EF.EventFrameRenderer(device="cpu")
    r = EF.EventFrameRenderer(True, 10, 98, 4, 4, "cuda")
    with pytest.raises(hip.V2ceHipError):
        r.add(0, torch.zeros(1, 2, 10, 4, 4))


def test_empty_clip_raises_like_the_host():
    """Nothing positive: np.percentile of an empty selection raises IndexError in event_frame_images; so does finish()."""
    with pytest.raises(IndexError):
        v2ce.event_frame_images(np.zeros((1, 3, 4, 4), np.float32), 10, 98, True)
    for keep in (True, False):
        with pytest.raises(IndexError):
            EF.EventFrameRenderer(keep, 10, 98, 4, 4, "cuda").finish()
    with pytest.raises(IndexError):
        R.frames(np.zeros((1, 3, 4, 4), np.float32), 10, 98, False, EF.percentile_from_order_stats)
