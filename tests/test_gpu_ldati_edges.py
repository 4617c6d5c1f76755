"""GPU parity of LDATI on voxel values at the branch points of the relocation recurrence ``ceil(y - debt - 1e-6)``: exact
integers, integer +- 1e-6, values below 1e-6, -0.0, the float below an integer, a subnormal, negative values, counts beyond
the slope table (tests/make_ldati_edge_goldens.py: edge_voxels).  csrc/ldati.hip restates the recurrence and the slope
parameters in about seven places (relocate_bins, relocate_all, the per-bin tile pass, the sparse tile kernel, both bodies of
the dense tile kernel, the sweep kernel, the fused count); every test here is bit-exact and is aimed at one of them.

Fixtures: the reference's own events (tests/golden/.ldati_edges), replayed with its uniforms.  Philox grids of the same
classes at 2 x 37 x 167 (three full 2048-pixel tiles per polarity plane plus one of 35 pixels) against the C oracle -- and at
2 x 36 x 172 (three tiles plus 48 pixels): 37 x 167 is odd, and the dense kernel's common-call body, like the 16-byte plane
loads of the count and sparse kernels, runs only where H W % 4 == 0 --, in two densities that follow from the plan's rules
(emit_impl):

  thin    edge_voxels(scale=0.4): no tile holds more than kSparseCap = 8192 events over its nine bins (about 6400 - 7200 here,
          asserted), so every tile is served by ldati_tile_sparse_kernel -- fused into the count pass on both calls of a
          stream, as a pass of its own with V2CE_LDATI_NO_FUSED=1; with V2CE_LDATI_NO_SPARSE=1 the tiles go to the dense kernel.
  thick   the classes over a 4 U[0,1) base: 28 000 - 32 000 events per full tile (asserted > kSparseCap), which takes
          ldati_tile_dense_kernel -- the two-pass path on the first call of a stream, the dense slot mode (the kernel is the
          count pass too) on the second --, or ldati_tile_pass_kernel with V2CE_LDATI_OLD_TILE=1 / V2CE_LDATI_NO_FASTDIV=1; the
          35-pixel tile stays with the sparse kernel.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ldati as O
from tests.make_ldati_edge_goldens import edge_voxels
from tests.test_gpu_ldati import hip_events, soa_equal
from tests.test_ldati_edges_cpu import CASES, load_case
from v2ce_toolbox_amd import LDATI, hip

pytestmark = pytest.mark.gpu

SEED, FRAME_BASE = 0xED6E5, 3
ALIGNED = (2, 36, 172)                      # H W % 4 == 0


def key_window(fps, t0):
    """[lo_c, lo_c + nk) microseconds per bin c: the key window of a bidirectional call as include/v2ce_hip.h documents it."""
    vs = 1.0 / fps / 9.0
    offt = [np.float32(c * vs) + np.float32(t0) for c in range(9)]
    assert all(o.dtype == np.float32 for o in offt)
    ulp_us = (abs(float(offt[8])) + vs) * 2.0 ** -23 * 1e6
    slack = 16 + int(8.0 * ulp_us)
    span = int(vs * 1e6) + 2
    return np.array([int(float(o) * 1e6) - slack - span for o in offt], np.int64), 3 * span + 2 * slack


def outside_window(want, fps, t0):
    """Per event of an oracle result: does its timestamp lie outside its bin's key window?  Also frame and bin per event."""
    seg, ts = want[0], want[1]
    lo, nk = key_window(fps, t0)
    c = np.repeat(np.tile(np.arange(9), seg.shape[0]), seg.reshape(-1))
    frame = np.repeat(np.arange(seg.shape[0]), seg.sum(axis=1))
    k = ts - lo[c]
    return (k < 0) | (k >= nk), frame


def zero_columns(vox, want, bad, frame):
    """vox with the (frame, polarity, pixel) columns of the events `bad` zeroed (polarity 0 = plane 1): without pooling a
    column's events depend on that column alone, so every other event stays what it was."""
    ok = np.array(vox, copy=True)
    ok[frame[bad], 1 - want[4][bad].astype(np.int64), :, want[3][bad].astype(np.int64), want[2][bad].astype(np.int64)] = 0
    return ok


FORWARD_UNPOOLED = ("slope", "slope_signed", "none", "fps60_t0", "int16")        # what path='sweep' serves
REPLAY = [(name, path, layout) for name in CASES for path in ("bucket", "sweep") for layout in ("packed", "soa")
          if path == "bucket" or name in FORWARD_UNPOOLED]


@pytest.mark.parametrize("name,path,layout", REPLAY)
def test_fixture_replay_matches_reference_and_oracle(name, path, layout):
    """Every fixture with the reference's uniforms.  The signed bidirectional one has events outside the key window of a
    bidirectional call (include/v2ce_hip.h: non-negative voxels only): it must be refused as it stands, and is compared with its
    offending (pixel, polarity) columns zeroed -- against the reference's records without those columns' events."""
    vox, u, fps, t0, strategy, opts, ref, lens = load_case(name)
    assert (name in FORWARD_UNPOOLED) == (not opts["bidirectional"] and opts["pooling_type"] == "none")
    assert path == "bucket" or hip.lib().v2ce_ldati_lds_bytes(fps, t0) != 0
    kw = dict(uniforms=u, strategy=strategy, **opts)
    want = O.emit_soa(vox, fps=fps, t0=t0, **kw)
    if opts["bidirectional"]:
        bad, frame = outside_window(want, fps, t0)
        assert bad.any() == (name == "bidir_signed")
        if bad.any():
            with pytest.raises(hip.V2ceHipError, match="left the key window"):
                hip_events(vox, fps, t0, path=path, layout=layout, **kw)
            assert opts["pooling_type"] == "none"
            vox = zero_columns(vox, want, bad, frame)
            # the reference's records of the other columns (its frames are `lens` long; polarity, y, x name the column)
            ref_frame = np.repeat(np.arange(len(lens)), lens)
            col = lambda f, p, y, x: ((f.astype(np.int64) * 2 + p) * vox.shape[3] + y) * vox.shape[4] + x
            gone = np.isin(col(ref_frame, ref["polarity"], ref["y"], ref["x"]), col(frame[bad], want[4][bad], want[3][bad], want[2][bad]))
            assert bad.sum() <= gone.sum() < 0.05 * len(ref)
            ref, lens = ref[~gone], np.bincount(ref_frame[~gone], minlength=len(lens))
            want = O.emit_soa(vox, fps=fps, t0=t0, **kw)
            assert not outside_window(want, fps, t0)[0].any()
    ev = hip_events(vox, fps, t0, path=path, layout=layout, **kw)
    # bit-exact vs the oracle, including the stable tie order
    soa_equal(ev, *want)
    # vs the reference's own output: exact up to the tie order its unstable argsort leaves open
    mine = np.concatenate(ev.to_recarrays())
    assert np.array_equal(ev.frame_counts, lens)
    assert np.array_equal(mine["timestamp"], ref["timestamp"])
    assert O.canonicalize(mine, ev.seg_counts.reshape(-1)).tobytes() == \
        O.canonicalize(ref, ev.seg_counts.reshape(-1)).tobytes()


def test_int16_grid_through_the_drop_in_call():
    """The reference's self-test input (LDATI.py:343): an int16 tensor handed to sample_voxel_statistical as it is."""
    vox, u, fps, t0, strategy, opts, ref, lens = load_case("int16")
    assert vox.dtype == np.int16
    y = torch.from_numpy(vox).cuda()
    assert y.dtype == torch.int16
    res = LDATI.sample_voxel_statistical(y, t0=t0, fps=fps, uniforms=torch.from_numpy(u))
    assert [len(r) for r in res] == lens.tolist()
    mine = np.concatenate(res)
    seg, _ = O.count(vox.astype(np.float32))
    assert mine.dtype == ref.dtype and np.array_equal(mine["timestamp"], ref["timestamp"])
    assert O.canonicalize(mine, seg.reshape(-1)).tobytes() == O.canonicalize(ref, seg.reshape(-1)).tobytes()


# ---------------------------------------------------------------------------------------------- Philox grids
@functools.lru_cache(maxsize=None)
def grid(density, signed, shape=(2, 37, 167)):
    B, H, W = shape
    kw = dict(scale=0.4) if density == "thin" else dict(uniform_base=4.0)
    vox = edge_voxels(np.random.default_rng(1000 + 2 * H + int(signed)), (B, 2, 10, H, W), signed, **kw)
    vox.setflags(write=False)
    return vox


@functools.lru_cache(maxsize=None)
def oracle(density, signed, fps=30, t0=0.0, shape=(2, 37, 167), strategy="slope", bidirectional=False, pooling_type="none",
           pooling_kernel_size=3):
    """The oracle's events for a grid, computed once and shared (read-only)."""
    out = O.emit_soa(grid(density, signed, shape), fps=fps, t0=t0, seed=SEED, frame_base=FRAME_BASE, strategy=strategy,
                     bidirectional=bidirectional, pooling_type=pooling_type, pooling_kernel_size=pooling_kernel_size)
    for a in out:
        a.setflags(write=False)
    return out


def tile_totals(want, shape):
    """Events per (frame, polarity, 2048-pixel tile) over the nine bins."""
    B, H, W = shape
    seg, ts, x, y, p = want
    tiles = (H * W + 2047) // 2048
    tot = np.zeros((B, 2, tiles), np.int64)
    frame = np.repeat(np.arange(B), seg.sum(axis=1))
    np.add.at(tot, (frame, 1 - p.astype(np.int64), (y.astype(np.int64) * W + x) // 2048), 1)     # (polarity 0 = plane 1)
    return tot


@pytest.mark.parametrize("signed", [False, True])
def test_grid_densities_are_what_the_docstring_says(signed):
    cap = LDATI._SPARSE_TILE_CAP
    assert cap == 8192
    thin, thick = tile_totals(oracle("thin", signed), (2, 37, 167)), tile_totals(oracle("thick", signed), (2, 37, 167))
    assert thin.shape == (2, 2, 4) and thin.max() <= cap and thin[..., :3].min() > cap // 2
    assert thick[..., :3].min() > 2 * cap and 0 < thick[..., 3].max() <= cap
    odd = tile_totals(oracle("thick", signed, shape=(2, 33, 47)), (2, 33, 47))
    assert odd.shape == (2, 2, 1) and odd.min() > cap and (33 * 47) % 4 != 0 and (37 * 167) % 4 != 0
    thin, thick = tile_totals(oracle("thin", signed, shape=ALIGNED), ALIGNED), tile_totals(oracle("thick", signed, shape=ALIGNED), ALIGNED)
    assert (36 * 172) % 4 == 0 and thin.shape == (2, 2, 4) and cap // 2 < thin[..., :3].min() and thin.max() <= cap
    assert thick[..., :3].min() > 2 * cap and 0 < thick[..., 3].max() <= cap


def run_twice(vox, want, fps=30, t0=0.0, **kw):
    """The first and the second call of a stream (no history: the fused count assumes sparse tiles; then with the first
    call's statistics), each bit-equal to the oracle."""
    LDATI._SEG_HINT.clear()
    for _ in range(2):
        soa_equal(hip_events(vox, fps, t0, seed=SEED, frame_base=FRAME_BASE, **kw), *want)


SWITCHES = ["OLD_TILE", "NO_SPARSE", "NO_FUSED", "NO_ATOMIC_ORDER", "NO_FASTDIV"]


@pytest.mark.parametrize("switch", [None] + SWITCHES)
@pytest.mark.parametrize("fps,t0", [(30, 0.0), (60, 0.5)])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("shape", [(2, 37, 167), ALIGNED], ids=["37x167", "36x172"])
@pytest.mark.parametrize("density", ["thin", "thick"])
def test_philox_edge_grids_equal_oracle(density, shape, signed, fps, t0, switch, monkeypatch):
    """The default path and each kernel-selection switch, first and second call of a stream."""
    if switch:
        monkeypatch.setenv("V2CE_LDATI_" + switch, "1")
    run_twice(grid(density, signed, shape), oracle(density, signed, fps, t0, shape), fps, t0)


@pytest.mark.parametrize("layout,path", [("soa", "bucket"), ("packed", "sweep"), ("soa", "sweep")])
@pytest.mark.parametrize("density", ["thin", "thick"])
def test_philox_edge_grids_other_layouts_and_sweep(density, layout, path):
    soa_equal(hip_events(grid(density, True), seed=SEED, frame_base=FRAME_BASE, layout=layout, path=path), *oracle(density, True))


def test_strategy_none_on_the_thick_signed_grid():
    run_twice(grid("thick", True), oracle("thick", True, strategy="none"), strategy="none")


@pytest.mark.parametrize("density,opts", [("thin", dict(strategy="random")),
                                          ("thin", dict(pooling_type="avg", pooling_kernel_size=5)),
                                          ("thick", dict(pooling_type="avg", pooling_kernel_size=5)),
                                          ("thin", dict(bidirectional=True)), ("thick", dict(bidirectional=True))],
                         ids=["thin-random", "thin-avg5", "thick-avg5", "thin-bidir", "thick-bidir"])
def test_options_on_the_non_negative_grid(density, opts):
    """('random' on the thin grid only: its generic path holds the tile pass's LDS plan for a key range of a whole second and
    refuses the thick grid's 5000 events per (tile, bin) with an error.)"""
    run_twice(grid(density, False), oracle(density, False, **opts), **opts)


@pytest.mark.parametrize("signed", [False, True])
def test_unaligned_planes_take_the_dense_kernels_scalar_load_body(signed):
    """H W % 4 != 0: no 16-byte plane loads."""
    shape = (2, 33, 47)
    run_twice(grid("thick", signed, shape), oracle("thick", signed, shape=shape))


@pytest.mark.parametrize("switches,path", [((), "bucket"), (("NO_FUSED",), "bucket"), (("NO_SPARSE",), "bucket"),
                                           (("NO_SPARSE", "NO_ATOMIC_ORDER"), "bucket"), (("NO_SPARSE", "OLD_TILE"), "bucket"),
                                           ((), "sweep")],
                         ids=["sparse-fused", "sparse", "dense-common-body", "dense-general-body", "per-bin", "sweep"])
def test_negative_neighbour_counts_beyond_2_24_take_the_slope_formula(switches, path, monkeypatch):
    """What the `n_l >= 0 && n_r >= 0` test in front of the slope table is for.  The table is indexed by the integer difference
    n_r - n_l; the reference forms float(n_r) - float(n_l) (LDATI.py:188, on y.float()).  The two agree while both counts are
    exact in f32.  A last-bin count is a SUM of two integers (LDATI.py:106): voxels of -2^24 around a multi-event voxel and -1
    in bin 9 give n_l = -2^24, n_r = -2^24 - 1, so the integer difference is -1 and the reference's is 0 (k == 0: another
    time formula).  Finite input, forward relocation: the oracle (which equals the reference on this column, checked when
    this test was written) must be matched by every kernel that looks the slope up."""
    vox = np.zeros((1, 2, 10, 4, 8), np.float32)
    rng = np.random.default_rng(5)
    vox[0, :, :, :2] = np.maximum(0.8 * rng.standard_normal((2, 10, 2, 8)), 0)
    for i, (pl, yy, xx) in enumerate([(0, 2, 1), (1, 2, 5), (0, 3, 0), (1, 3, 7), (0, 3, 4)]):
        vox[0, pl, :, yy, xx] = [0.3, 0, 1.0, 0, 0, 0, -2.0 ** 24, 2.5 + i, -2.0 ** 24, -1.0]
    n, _ = O.relocate(vox[0, 0, :, 2, 1])
    assert n.tolist()[6:] == [-2 ** 24, 3, -2 ** 24 - 1]
    for sw in switches:
        monkeypatch.setenv("V2CE_LDATI_" + sw, "1")
    want = O.emit_soa(vox, seed=SEED, frame_base=FRAME_BASE)
    LDATI._SEG_HINT.clear()
    for _ in range(2):
        soa_equal(hip_events(vox, seed=SEED, frame_base=FRAME_BASE, path=path), *want)


def test_batching_invariance_on_the_signed_grid():
    vox = grid("thick", True, (3, 37, 167))
    whole = hip_events(vox, seed=SEED, frame_base=100)
    a = hip_events(vox[:1], seed=SEED, frame_base=100)
    b = hip_events(vox[1:], seed=SEED, frame_base=101)
    assert np.array_equal(whole.seg_counts, np.concatenate([a.seg_counts, b.seg_counts]))
    for f in ("ts", "x", "y", "p"):
        assert np.array_equal(getattr(whole, f).cpu().numpy(),
                              np.concatenate([getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()])), f


# ---------------------------------------------------------------------------------------------- signed + bidirectional
@pytest.mark.parametrize("fps,t0", [(30, 0.0), (60, 0.5)])
@pytest.mark.parametrize("density", ["thin", "thick"])
def test_non_negative_bidirectional_grids_stay_inside_the_key_window(density, fps, t0):
    bad, _ = outside_window(oracle(density, False, fps, t0, bidirectional=True), fps, t0)
    assert not bad.any()


@pytest.mark.parametrize("fps,t0", [(30, 0.0), (60, 0.5)])
@pytest.mark.parametrize("density,switch", [("thin", None), ("thin", "NO_FUSED"), ("thick", None), ("thick", "NO_SPARSE")])
def test_signed_bidirectional_grid_is_refused_not_clamped(density, switch, fps, t0, monkeypatch):
    """Bidirectional relocation of a grid with negative voxels: some single-event tendencies (bin 8's is y[9] itself) lie
    outside the key window, which is sized for non-negative grids.  The device used to clamp such a key -- a wrong timestamp,
    silently.  Now the call is refused: by the sparse tile kernel as part of the fused count (thin), as a pass of its own
    (thin, NO_FUSED), by the per-bin tile kernel (thick; all tiles with NO_SPARSE).  With the offending (pixel, polarity)
    columns zeroed the same grid is served bit-exactly."""
    if switch:
        monkeypatch.setenv("V2CE_LDATI_" + switch, "1")
    vox = grid(density, True)
    want = oracle(density, True, fps, t0, bidirectional=True)
    bad, frame = outside_window(want, fps, t0)
    assert 10 <= bad.sum() < 0.01 * bad.size
    LDATI._SEG_HINT.clear()
    for _ in range(2):
        with pytest.raises(hip.V2ceHipError, match="left the key window"):
            hip_events(vox, fps, t0, seed=SEED, frame_base=FRAME_BASE, bidirectional=True)
    ok = zero_columns(vox, want, bad, frame)
    assert (ok < 0).any()
    want_ok = O.emit_soa(ok, fps=fps, t0=t0, seed=SEED, frame_base=FRAME_BASE, bidirectional=True)
    assert not outside_window(want_ok, fps, t0)[0].any()
    run_twice(ok, want_ok, fps, t0, bidirectional=True)


def test_signed_bidirectional_random_is_refused_on_the_generic_path():
    want = oracle("thin", True, strategy="random", bidirectional=True)
    seg, ts = want[0], want[1]
    lo, nk = key_window(30, 0.0)
    c = np.repeat(np.tile(np.arange(9), 2), seg.reshape(-1))
    k = ts - lo[c]
    assert ((k < 0) | (k >= nk + 1000000)).any()                # ('random': a second of raw uniforms on top of the window)
    with pytest.raises(hip.V2ceHipError, match="left the key window"):
        hip_events(grid("thin", True), seed=SEED, frame_base=FRAME_BASE, strategy="random", bidirectional=True)
