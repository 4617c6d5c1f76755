"""GPU: the ablation samplers (csrc/sampler.hip) where test_gpu_samplers.py never goes: boundary voxel values, planted columns
and boundary draws against the reference's own events (tests/golden/.sampler_edges), key field widths and block edges,
Philox counters beyond the first word, timestamp ties, and voxels for which the reference's result is not defined.
Bit-exact throughout.  Every case prints one line ``SAMPLER-EDGE <name> events=<n> classes=<...>``."""
import functools

import numpy as np
import pytest

from oracle import sample_methods as OS
from tests import make_sampler_edge_goldens as G
from tests import test_gpu_samplers as TS
from tests import test_sampler_edges_cpu as EC
from v2ce_toolbox_amd import hip

pytestmark = pytest.mark.gpu
MODES = [("baseline", "random"), ("baseline", "even"), ("pure_slope", "slope")]


def report(name, res, vox, kind):
    masks = G.classes(G.effective(vox, kind))
    cls = {k: int(m.sum()) for k, m in masks.items()}
    cls["negative"] = int((np.asarray(vox) < 0).sum())
    print(f"SAMPLER-EDGE {name} events={sum(len(r) for r in res)} classes={cls}")


def cross_pixel_ties(res):
    """Neighbours in the output with the same timestamp and another pixel."""
    n = 0
    for r in res:
        r = np.asarray(r)
        n += int(((np.diff(r["timestamp"]) == 0) & ((np.diff(r["x"]) != 0) | (np.diff(r["y"]) != 0))).sum())
    return n


# ---- a. the reference's fixtures, replayed draws
@pytest.mark.parametrize("name", EC.CASES)
def test_reference_edge_fixtures(gold_dir, name):
    z = EC.load_case(gold_dir, name)
    draws = dict(u_int=z["u_int"], u_dec=z["u_dec"], u_bern=z["u_bern"])
    res = TS.run_device(z["vox"], z["kind"], z["mode"], z["t0"], z["fps"], **draws, **z["opts"])
    print(f"SAMPLER-EDGE {name} events={sum(len(r) for r in res)} classes={dict(zip(G.CLASSES, z['class_events'].tolist()))} "
          f"planted={dict(zip(G.PLANTED, z['planted_events'].tolist()))}")
    assert [len(r) for r in res] == z["lens"].tolist()
    if name in G.POOLED:
        lo = 0
        for r in res:
            d = OS.events_close(np.asarray(r), z["ref"][lo:lo + len(r)])
            assert 0 <= d <= len(r) // 1000, d
            lo += len(r)
        TS.same(res, EC.oracle_of(z))
    else:
        assert np.concatenate([np.asarray(r) for r in res]).tobytes() == z["events"].tobytes()
    TS.same(res, TS.run_device(z["vox"], z["kind"], z["mode"], z["t0"], z["fps"], **draws, **z["opts"]))
    first = TS.run_device(z["vox"][:1], z["kind"], z["mode"], z["t0"], z["fps"], **{k: v[:1] for k, v in draws.items()}, **z["opts"])
    TS.same(first, res[:1])


# ---- b. key field widths and block edges
ROWS = [(1, 1, 1, 30, 0.0), (1, 1, 2, 24, 1e-3), (2, 1, 63, 30, 0.0), (1, 5, 51, 1000, 0.0), (4, 64, 4, 30, 0.0),
        (1, 1, 257, 31.7, -0.01), (3, 2, 256, 1, -0.75), (2, 128, 1, 1000, 3600.0), (5, 129, 257, 1, 3600.0)]


@functools.lru_cache(maxsize=1)
def row_inputs(row):
    B, H, W, _, _ = row
    rng = np.random.default_rng([B, H, W])
    vox, _ = G.edge_voxels(rng, (B, 2, 10, H, W), max_count=3)
    if H * W == 1:
        vox[0, 0, :, 0, 0] = np.minimum(G.planted_columns()["ramp_up"], [3.75] * 8 + [1.875] * 2)    # (too few columns to plant any)
    M = EC.max_count(vox)
    assert M <= 3
    return vox, dict(zip(("u_int", "u_dec", "u_bern"), EC.numpy_draws(rng, vox.shape, M)))


@pytest.mark.parametrize("kind,mode", MODES)
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "B%dxH%dxW%d-fps%g-t0%g" % r)
def test_key_widths_and_block_edges(row, kind, mode):
    B, H, W, fps, t0 = row
    vox, draws = row_inputs(row)
    want = TS.run_oracle(vox, kind, mode, t0, fps, **draws)
    got = TS.run_device(vox, kind, mode, t0, fps, **draws)
    ties = cross_pixel_ties(got)
    report(f"B{B}xH{H}xW{W}-fps{fps:g}-t0{t0:g}-{mode} cross_pixel_ties={ties}", got, vox, kind)
    TS.same(got, want)
    assert sum(len(r) for r in got) > 0
    if t0 == 3600.0:            # f32 timestamps in steps of 256 us: ordered by the x / y / polarity fields of the key alone
        assert ties > 100


# ---- c. Philox at the counter edges
@functools.lru_cache(maxsize=None)
def philox_inputs(variant):
    shape = (1, 2, 10, 2, 35)
    vox, _ = G.edge_voxels(np.random.default_rng(811), shape, max_count=3)
    big = (0, 10) if variant == "middle" else (1, 28)          # pixel 10, or pixel 63: the last lane of the first wave
    if variant == "last_lane":
        vox[:, :, :, 1, 29:] = 0                               # pixels 64..69: the second wave of both planes is empty
    vox[0, 0, 3, big[0], big[1]] = 300.25
    vox[0, 1, 8, 0, 20] = 5.5
    vox[0, 1, 9, 0, 20] = 0
    return vox


@functools.lru_cache(maxsize=1)
def philox_uniforms():
    return OS.philox_draws(1, 2, 35, 300, seed=4242, frame_base=7)


@pytest.mark.parametrize("kind,mode", [("baseline", "random"), ("pure_slope", "slope")])
@pytest.mark.parametrize("variant", ["middle", "last_lane"])
def test_philox_counter_words(variant, kind, mode):
    """300 events in one voxel: draws j = 0..299 come from counter words j >> 2 = 0..74, lanes j & 3."""
    vox = philox_inputs(variant)
    assert EC.max_count(vox) == 300
    u_int, u_dec, u_bern = philox_uniforms()
    want = TS.run_oracle(vox, kind, mode, 0.0, 30, u_int=u_int, u_dec=u_dec, u_bern=u_bern)
    got = TS.run_device(vox, kind, mode, 0.0, 30, seed=4242, frame_base=7)
    report(f"philox-{variant}-{mode}", got, vox, kind)
    TS.same(got, want)
    assert len(got[0]) > 305
    if variant == "last_lane":
        r = np.asarray(got[0])
        assert not (r["x"].astype(int) + 35 * r["y"].astype(int) >= 64).any()


# ---- d. ties
def test_even_ties_are_ordered_by_the_low_key_fields():
    B, H, W = 2, 3, 5
    vox = np.full((B, 2, 10, H, W), 3.0, np.float32)
    u_bern = EC.numpy_draws(np.random.default_rng(5), vox.shape, 0)[2]
    want = TS.run_oracle(vox, "baseline", "even", 0.0, 30, u_bern=u_bern)
    got = TS.run_device(vox, "baseline", "even", 0.0, 30, u_bern=u_bern)
    report("ties-even", got, vox, "baseline")
    TS.same(got, want)
    a, b = np.asarray(got[0]), np.asarray(got[1])
    assert a.tobytes() == b.tobytes() and len(a) == 3 * 2 * 10 * H * W
    ts, counts = np.unique(a["timestamp"], return_counts=True)
    assert len(ts) == 30 and (counts == 2 * H * W).all()                     # every time is shared by all pixels and planes
    group = a[:2 * H * W]
    assert group["x"].tolist() == np.repeat(np.arange(W), 2 * H).tolist()
    assert group["y"].tolist() == np.tile(np.repeat(np.arange(H), 2), W).tolist()
    assert group["polarity"].tolist() == [0, 1] * (H * W)
    key = (((a["timestamp"] * 64 + a["x"]) * 64) + a["y"]) * 2 + a["polarity"]
    assert (np.diff(key) > 0).all()


# ---- e. unphysical but finite voxels
@pytest.mark.parametrize("name", list(EC.UNPHYSICAL))
def test_unphysical_voxels(name):
    """Negative voxels: where every selected time is finite and near the frame the device gives the oracle's bytes; where
    one is NaN / inf (the reference's cast to int64 has no defined result) the call raises and returns nothing."""
    vox, kind, mode, fps, t0, draws, want = EC.unphysical_case(name)
    us = OS.selected_times_us(vox, kind, mode, t0, fps, **draws)
    assert EC.classify(us, fps, t0) == want
    print(f"SAMPLER-EDGE unphysical-{name} class={want} events={len(us)} classes={{'negative': {int((vox < 0).sum())}, "
          f"'nan': {int(np.isnan(us).sum())}, 'inf': {int(np.isinf(us).sum())}}}")
    if want == "undefined":
        with pytest.raises(hip.V2ceHipError, match="timestamp"):
            TS.run_device(vox, kind, mode, t0, fps, **draws)
        return
    try:
        got = TS.run_device(vox, kind, mode, t0, fps, **draws)
    except hip.V2ceHipError:
        assert want == "between"
        print(f"SAMPLER-EDGE unphysical-{name} refused by the key window")
        return
    TS.same(got, TS.run_oracle(vox, kind, mode, t0, fps, **draws))
    assert len(got[0]) == len(us) > 0
