"""CPU: the oracle of the two ablation samplers (oracle/sample_methods.py) on the boundary fixtures of
tests/make_sampler_edge_goldens.py (tests/golden/.sampler_edges): exact integers, floats below integers, zeros, tiny values,
the planted fold / flat / ramp / one-hot columns and draws of exactly 0 and 1 - 2^-24 -- against the REFERENCE's own events
for them, and the conditions under which those fixtures exercise what they are meant to."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import sample_methods as OS
from tests import make_sampler_edge_goldens as G
from tests.test_oracle_goldens_recipe import _compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = ".sampler_edges"
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
CASES = list(G.CASES)


def load_case(gold_dir, name):
    z = dict(np.load(os.path.join(gold_dir, DIR, f"sampler_edges_{name}.npz")))
    z["opts"] = {} if str(z["pooling_type"]) == "none" else \
        dict(pooling_type=str(z["pooling_type"]), pooling_kernel_size=int(z["pooling_kernel_size"]))
    z["ref"] = np.frombuffer(z["events"].tobytes(), OS.EVENT_DTYPE)
    for k in ("kind", "mode"):
        z[k] = str(z[k])
    for k in ("fps", "t0"):
        z[k] = float(z[k])
    return z


def oracle_of(z):
    return G.run_oracle(z["vox"], z["kind"], z["mode"], z["fps"], z["t0"], z["opts"], z["u_int"], z["u_dec"], z["u_bern"])


def voxel_events_of(z):
    return G.voxel_events(z["vox"], z["kind"], z["mode"], z["fps"], z["t0"], z["opts"], z["u_int"], z["u_dec"], z["u_bern"])


def test_goldens_present(gold_dir):
    files = sorted(glob.glob(os.path.join(gold_dir, DIR, "*")))
    assert [os.path.basename(f) for f in files] == sorted(f"sampler_edges_{c}.npz" for c in CASES)
    for f in files:
        assert os.path.getsize(f) <= G.MAX_BYTES, f
    for name in CASES:
        kind, mode, shape, fps, t0, opts, _ = G.CASES[name]
        z = load_case(gold_dir, name)
        assert (z["kind"], z["mode"], z["vox"].shape, z["fps"], z["t0"]) == (kind, mode, shape, fps, t0)
        assert z["opts"] == ({} if not opts else {"pooling_kernel_size": 3, **opts})


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference(gold_dir, name):
    z = load_case(gold_dir, name)
    res = oracle_of(z)
    assert [len(r) for r in res] == z["lens"].tolist()
    if name in G.POOLED:          # the bar of test_pooled_pure_slope_close_to_reference
        lo = 0
        for r in res:
            d = OS.events_close(np.asarray(r), z["ref"][lo:lo + len(r)])
            assert 0 <= d <= len(r) // 1000, d
            lo += len(r)
    else:
        got = np.concatenate([np.asarray(r) for r in res])
        assert got.dtype.itemsize == 13 and got.tobytes() == z["events"].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_integer_voxels_and_columns(gold_dir, name):
    """Per (frame, pixel, polarity) the reference's events number sum_c floor(y) + [u_bern < frac(y)], with no Bernoulli
    event on an exact integer although draws of exactly 0 sit on some; bin 9 of the pure-slope kind is silent."""
    z = load_case(gold_dir, name)
    vox, ref = z["vox"], z["ref"]
    B, _, _, H, W = vox.shape
    eff = G.effective(vox, z["kind"])
    assert vox.dtype == np.float32 and np.isfinite(vox).all() and (vox >= 0).all()
    per_voxel, n, sel, _ = voxel_events_of(z)
    integer = eff == np.rint(eff)
    assert np.array_equal(n, np.floor(eff)) and not sel[integer].any()
    assert np.array_equal(per_voxel[integer], eff[integer])                   # exactly floor(y) events, u_bern == 0 or not
    if name != "slope_odd_fps":                                               # (180 voxels: the 2 % may miss the integers)
        assert ((z["u_bern"] == 0) & integer).any()
    want = per_voxel.sum(axis=2)                                              # [B, 2, H, W]
    got = np.zeros_like(want)
    frame = np.repeat(np.arange(B), z["lens"])
    np.add.at(got, (frame, 1 - ref["polarity"].astype(np.int64), ref["y"].astype(np.int64), ref["x"].astype(np.int64)), 1)
    assert np.array_equal(got, want)
    if z["kind"] == "pure_slope":
        assert not per_voxel[:, :, 9].any() and vox[:, :, 9].any()


def test_classes_and_planted_columns(gold_dir):
    """The generator's conditions, read from the files: every class and planted column occurs in every case and emits in
    at least one case of its kind; zeros emit nothing; planted draws of 0 and of 1 - 2^-24 stand behind emitted events."""
    seen = {}
    for name in CASES:
        z = load_case(gold_dir, name)
        kind = z["kind"]
        assert tuple(z["class_names"]) == G.CLASSES and tuple(z["planted_names"]) == G.PLANTED
        eff = G.effective(z["vox"], kind)
        masks = G.classes(eff)
        per_voxel, _, _, used = voxel_events_of(z)
        assert z["class_voxels"].tolist() == [int(masks[k].sum()) for k in G.CLASSES] and z["class_voxels"].min() > 0
        assert z["class_events"].tolist() == [int(per_voxel[masks[k]].sum()) for k in G.CLASSES]
        cols = G.planted_columns()
        for i, (k, (b, pi, h, w)) in enumerate(zip(G.PLANTED, z["planted_at"])):
            assert np.array_equal(z["vox"][b, pi, :, h, w], cols[k]), (name, k)
            assert z["planted_events"][i] == per_voxel[b, pi, :, h, w].sum()
            seen[kind, k] = seen.get((kind, k), 0) + int(z["planted_events"][i])
        for k, e in zip(G.CLASSES, z["class_events"]):
            seen[kind, k] = seen.get((kind, k), 0) + int(e)
        for k, v in (("u0", used == 0), ("utop", used == G.TOP)):
            seen[kind, k] = seen.get((kind, k), 0) + int(v.sum())
        if kind == "pure_slope":           # the fold: bin 8 of fold_cross holds 1.2, of fold_zero 3.0
            b, pi, h, w = z["planted_at"][G.PLANTED.index("fold_cross")]
            assert per_voxel[b, pi, 8, h, w] >= 1
            b, pi, h, w = z["planted_at"][G.PLANTED.index("fold_zero")]
            assert per_voxel[b, pi, 8, h, w] == 3 and z["vox"][b, pi, 8, h, w] == 0
    for kind in ("baseline", "pure_slope"):
        for k in G.CLASSES + G.PLANTED + ("u0", "utop"):
            assert (seen[kind, k] == 0) == (k == "zero"), (kind, k)


@pytest.mark.parametrize("name", CASES)
def test_timestamps_inside_the_smallest_key_window(gold_dir, name):
    """4096 us is the smallest margin csrc/sampler.hip ever adds around [t0, t0 + 1/fps]: no fixture may be refused."""
    z = load_case(gold_dir, name)
    lo, hi = z["t0"] * 1e6, z["t0"] * 1e6 + 1e6 / z["fps"]
    ts = z["ref"]["timestamp"]
    assert len(ts) and lo - 4096 <= ts.min() and ts.max() <= hi + 4096, (ts.min() - lo, ts.max() - hi)
    us = OS.selected_times_us(z["vox"], z["kind"], z["mode"], z["t0"], z["fps"], u_int=z["u_int"], u_dec=z["u_dec"],
                              u_bern=z["u_bern"], **z["opts"])
    assert len(us) == len(ts) and np.isfinite(us).all()
    assert np.array_equal(np.sort(us.astype(np.int64)), np.sort(ts)) or name in G.POOLED


# ---- unphysical but finite voxels (negative values): which calls have a defined result at all
NEG_M1 = np.array([1.0, 2.5, 0.0, 1.0, -0.5, 1.0, 0.3, 0.0, 1.5, 0.25], np.float32)            # floor(y4) == -1
NEG_EPS_EQ = np.array([0.5, 1.0, 2.0, 1.0, -1e-8, 1.0, 0.0, 0.75, 0.5, 0.0], np.float32)       # y4 + 1e-8 == 0, y3 == y5
NEG_EPS_NE = np.array([0.5, 1.0, 2.0, 0.5, -1e-8, 2.0, 0.0, 0.75, 0.5, 0.0], np.float32)       # the same, y3 != y5
# name: (kind, mode, fps, t0, negative voxels are -U(lo, hi), planted column or None, class)
UNPHYSICAL = {
    "random_neg": ("baseline", "random", 30, 0.0, (0, 3), None, "defined"),
    "slope_neg": ("pure_slope", "slope", 30, 0.0, (0, 3), None, "defined"),
    "slope_neg_late": ("pure_slope", "slope", 25, 1.5, (0, 3), None, "defined"),
    "even_below_m1_fps1000": ("baseline", "even", 1000, 0.0, (1, 3), None, "defined"),       # <= 2 bins of 100 us late
    "even_m1_t0": ("baseline", "even", 30, 0.0, (0, 3), NEG_M1, "undefined"),                # -1 / 0
    "even_m1_t1.5": ("baseline", "even", 30, 1.5, (0, 3), NEG_M1, "undefined"),
    "slope_eps_eq_t0": ("pure_slope", "slope", 30, 0.0, (0, 3), NEG_EPS_EQ, "undefined"),    # k = 0 / 0
    "slope_eps_eq_t1.5": ("pure_slope", "slope", 30, 1.5, (0, 3), NEG_EPS_EQ, "undefined"),
    "slope_eps_ne_t0": ("pure_slope", "slope", 30, 0.0, (0, 3), NEG_EPS_NE, "undefined"),    # k = x / 0
    "slope_eps_ne_t1.5": ("pure_slope", "slope", 30, 1.5, (0, 3), NEG_EPS_NE, "undefined"),
    "even_below_m1_fps1": ("baseline", "even", 1, 0.0, (1, 3), None, "between"),             # <= 2 bins of 0.1 s late
}


def numpy_draws(rng, shape, M):
    """24-bit uniforms as torch.rand gives them, about 2 % of the time draws planted at 0 / 1 - 2^-24 and of the
    Bernoulli draws at 0."""
    def uni(sh):
        u = (rng.integers(0, 1 << 24, sh).astype(np.float32) * np.float32(2.0 ** -24))
        pick = rng.random(sh)
        return u, pick
    B, _, _, H, W = shape
    u_int, pick = uni((B, 2, 10, H, W, M))
    u_int[pick < 0.01], u_int[pick >= 0.99] = 0, G.TOP
    u_dec, pick = uni((B, 2, 10, H, W))
    u_dec[pick < 0.01], u_dec[pick >= 0.99] = 0, G.TOP
    u_bern, pick = uni((B, 2, 10, H, W))
    u_bern[pick < 0.02] = 0
    return u_int, u_dec, u_bern


def max_count(vox):
    return max(int(np.floor(G.effective(vox, "pure_slope")).max()), int(np.floor(vox).max()), 0)


def unphysical_case(name):
    """-> (vox, kind, mode, fps, t0, draws, class expected).  1 x 2 x 10 x 4 x 6, counts <= 3, about 1/10 negative."""
    kind, mode, fps, t0, (lo, hi), col, want = UNPHYSICAL[name]
    rng = np.random.default_rng(sorted(UNPHYSICAL).index(name) + 700)
    shape = (1, 2, 10, 4, 6)
    vox, _ = G.edge_voxels(rng, shape, max_count=3)
    neg = -(lo + (hi - lo) * rng.random(shape)).astype(np.float32)
    vox = np.where(rng.integers(0, 10, shape) == 0, neg, vox).astype(np.float32)
    draws = numpy_draws(rng, shape, max_count(vox))
    if col is not None:
        vox[0, 1, :, 2, 3] = col
        draws[2][0, 1, :, 2, 3] = 0                  # the Bernoulli event of every fractional bin of the column exists
    assert np.isfinite(vox).all() and (vox < 0).sum() >= 20
    return vox, kind, mode, fps, t0, dict(zip(("u_int", "u_dec", "u_bern"), draws)), want


def classify(us, fps, t0):
    """From the pre-cast f32 microsecond times of the selected events: 'undefined' (some NaN / inf: the cast to int64 has
    no defined result), 'defined' (all within 4096 us of the frame interval, the smallest margin of the key window) or
    'between'."""
    if not np.isfinite(us).all():
        return "undefined"
    lo, hi = t0 * 1e6, t0 * 1e6 + 1e6 / fps
    return "defined" if len(us) and lo - 4096 <= us.min() and us.max() <= hi + 4096 else "between"


@pytest.mark.parametrize("name", list(UNPHYSICAL))
def test_unphysical_cases_fall_into_their_class(name):
    vox, kind, mode, fps, t0, draws, want = unphysical_case(name)
    us = OS.selected_times_us(vox, kind, mode, t0, fps, **draws)
    assert classify(us, fps, t0) == want
    if want == "undefined" and mode == "slope":            # the planted voxel alone: every other selected time is fine
        assert np.isnan(us).sum() == 1 and np.isfinite(us).sum() == len(us) - 1
    assert sum(c[-1] == "between" for c in UNPHYSICAL.values()) <= 1


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "train", "scripts", "stage2", "sample_methods", "pure_slope_sample.py")),
                    reason="the reference tree is not on this machine")
def test_recipe_regenerates_fixtures(tmp_path):
    out = tmp_path / DIR
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "make_sampler_edge_goldens.py"), str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    made = sorted(os.listdir(out))
    assert made == sorted(os.listdir(os.path.join(ROOT, "tests", "golden", DIR)))
    _compare(str(tmp_path), [os.path.join(DIR, f) for f in made])
