"""Recipe of tests/golden/.sampler_edges/sampler_edges_<case>.npz: the two ablation samplers (random / even baseline, pure
slope) on voxel values, planted columns and random draws at the branch points of csrc/sampler.hip -- the REFERENCE's own events
for them, with every draw it used.

The grids of the sampler_g10* fixtures come from continuous distributions, in which none of this occurs.  Here each class
replaces about 1/10 of the voxels of a ``relu(0.8 randn)`` base (edge_voxels()):

    integer     exact 0..4                      frac == 0: no Bernoulli event, not even for a draw of exactly 0 (u < 0)
    below       nextafter(i + 1, 0), i in 0..3  frac == 1 - 2^-24 .. 1 - 2^-22
    zero        0
    tiny        U(0, 2e-6)

classes() counts them BY VALUE on the grid the sampler splits into floor and fraction (for the pure-slope kind: bin 9 folded
into bin 8), so an ``integer`` drawn as 0 counts as ``zero``.  Six columns (one pixel, one polarity plane, all ten bins) are
planted on top (PLANTED): fold_cross (y8 = y9 = 0.6: the fold crosses an integer when neither term does), fold_zero (y8 = 0,
y9 = 3: events in bin 8 whose slope comes from the unfolded y8 + 1e-8, k ~ 1e13), flat (k == 0 in every bin), ramp_up and
ramp_down (k > 0, k < 0; k == 0 at both reflected ends), one_hot (40 events in one voxel between empty ones).

Draws: torch.rand is wrapped so that about 2 % of every tensor the reference draws for event times become exactly 0 or
1 - 2^-24 (the extremes of a 24-bit uniform) and about 2 % of the Bernoulli draws exactly 0, BEFORE the reference uses them:
the fixture holds what the reference actually used.

As in oracle/make_goldens.py (whose DrawCapture, IeeeSqrt, reference import and Bernoulli plane order are used here, not
copied) a torch seed is searched for which the reference gives the same bytes with this torch build's MKL sqrt and with an
IEEE sqrt; the pooled cases run with the IEEE sqrt and are held to 1 us against the oracle, as the g10p fixtures are.  The
files hold the arrays of the sampler_g10_* fixtures plus the pooling options, the class counts and the planted columns; to
stay below 250 KB the ``u_int`` draws the reference never reads (index >= the voxel's count) are stored as 0 and the last
axis stops at the largest count.  tests/golden/'s top level is exactly the output set of oracle/make_goldens.py, so these sit
in a dot directory that it skips.  Runs where the reference tree is present; not collected by pytest.

    python tests/make_sampler_edge_goldens.py [out_dir]      (default tests/golden/.sampler_edges)
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import sample_methods as OS                     # noqa: E402

F = np.float32
TOP = F(1) - F(2.0 ** -24)                                  # the largest value of a 24-bit uniform
CLASSES = ("integer", "below", "zero", "tiny")
PLANTED = ("fold_cross", "fold_zero", "flat", "ramp_up", "ramp_down", "one_hot")
ONE_HOT = 40.0
MAX_BYTES = 250 * 1024
# name: (kind, mode, shape, fps, t0, pooling options, seed of the grid)
CASES = {
    "random": ("baseline", "random", (2, 2, 10, 5, 7), 30, 0.0, {}, 601),
    "even": ("baseline", "even", (2, 2, 10, 5, 7), 1, -0.75, {}, 602),
    "even_late": ("baseline", "even", (2, 2, 10, 5, 7), 1000, 3600.0, {}, 603),
    "slope": ("pure_slope", "slope", (2, 2, 10, 5, 7), 30, 0.0, {}, 604),
    "slope_odd_fps": ("pure_slope", "slope", (1, 2, 10, 1, 9), 31.7, -0.01, {}, 605),
    "slope_late": ("pure_slope", "slope", (2, 2, 10, 5, 7), 1, 3600.0, {}, 606),
    "slope_weighted": ("pure_slope", "slope", (2, 2, 10, 5, 7), 30, 0.0, dict(pooling_type="weighted"), 607),
    "slope_avg7": ("pure_slope", "slope", (2, 2, 10, 5, 7), 30, 0.0, dict(pooling_type="avg", pooling_kernel_size=7), 608),
}
POOLED = tuple(n for n, c in CASES.items() if c[5])


def planted_columns():
    ramp = 0.5 * (np.arange(10) + 1)
    cols = {
        "fold_cross": [0.3, 1.2, 0.0, 2.5, 0.7, 0.0, 1.1, 0.4, 0.6, 0.6],
        "fold_zero": [0.0, 1.5, 0.2, 0.0, 2.0, 0.8, 0.0, 1.25, 0.0, 3.0],
        "flat": [2.0] * 10,
        "ramp_up": ramp,
        "ramp_down": ramp[::-1],
        "one_hot": [0.0] * 4 + [ONE_HOT] + [0.0] * 5,
    }
    return {k: np.asarray(v, F) for k, v in cols.items()}


def class_values(rng, n):
    """n voxel values: a relu(0.8 randn) base, each class drawn for about 1/10 of them."""
    v = np.maximum(0.8 * rng.standard_normal(n), 0.0).astype(F)
    cls = rng.integers(0, 10, n)
    ints = rng.integers(0, 5, n).astype(F)
    below = np.nextafter((rng.integers(0, 4, n) + 1).astype(F), F(0))
    tiny = (rng.random(n) * 2e-6).astype(F)
    v = np.where(cls == 0, ints, v)
    v = np.where(cls == 1, below, v)
    v = np.where(cls == 2, F(0), v)
    v = np.where(cls == 3, tiny, v)
    return v.astype(F)


def edge_voxels(rng, shape, max_count=None):
    """-> ([B,2,10,H,W] f32 grid, [6,4] int (frame, plane, h, w) of the planted columns in PLANTED's order).
    ``max_count`` caps every value at max_count + 0.75 and bins 8 and 9 at half of that, so that no voxel and no fold holds
    more than max_count events (the GPU tests' large grids: the oracle's draw tensor stays small)."""
    B, P, C, H, W = shape
    v = class_values(rng, int(np.prod(shape))).reshape(shape)
    cols = rng.choice(B * P * H * W, len(PLANTED), replace=False) if B * P * H * W >= len(PLANTED) else []
    at = np.zeros((len(cols), 4), np.int64)
    for i, (name, col) in enumerate(zip(PLANTED, cols)):
        b, pi, h, w = np.unravel_index(col, (B, P, H, W))
        v[b, pi, :, h, w] = planted_columns()[name]
        at[i] = b, pi, h, w
    if max_count is not None:
        v = np.minimum(v, F(max_count + 0.75))
        v[:, :, 8:] = np.minimum(v[:, :, 8:], F((max_count + 0.75) / 2))
    return v, at


def effective(vox, kind):
    """The grid whose floor and fraction decide the events: pure slope folds bin 9 into bin 8 first."""
    v = np.array(vox, F)
    if kind == "pure_slope":
        v[:, :, 8] = v[:, :, 8] + v[:, :, 9]
        v[:, :, 9] = 0
    return v


def classes(eff):
    """name -> boolean mask over the effective grid, by value."""
    r = np.rint(eff)
    return {
        "integer": (eff == r) & (eff >= 1) & (eff <= 4),
        "below": (eff == np.nextafter(r.astype(F), F(0))) & (r >= 1) & (r <= 4),
        "zero": eff == 0,
        "tiny": (eff > 0) & (eff < 2e-6),
    }


def voxel_events(vox, kind, mode, fps, t0, opts, u_int, u_dec, u_bern):
    """Events per voxel [B,2,10,H,W] and the draws behind them (floor-event draws that are read; Bernoulli-time draws of
    the hits), from the oracle's own selection."""
    if kind == "baseline":
        _, ip, _, sel = OS._baseline_parts(vox, t0, fps, mode == "even", mode == "random", u_int, u_dec, u_bern)
    else:
        _, ip, _, sel = OS._pure_slope_parts(vox, t0, fps, opts.get("pooling_type", "none"),
                                             opts.get("pooling_kernel_size", 3), u_int, u_dec, u_bern)
    n = np.maximum(ip, 0).astype(np.int64)
    read = np.arange(u_int.shape[-1]) < n[..., None]
    used = np.concatenate([u_int[read], u_dec[sel]]) if mode != "even" else np.zeros(0, F)
    return n + sel, n, sel, used


def run_oracle(vox, kind, mode, fps, t0, opts, u_int, u_dec, u_bern):
    kw = dict(u_int=u_int, u_dec=u_dec, u_bern=u_bern)
    if kind == "baseline":
        return OS.sample_voxel_baseline(vox, t0, fps, even=mode == "even", random=mode == "random", **kw)
    return OS.sample_voxel_pure_slope(vox, t0, fps, **opts, **kw)


def main(out_dir):
    import torch
    from oracle import make_goldens as MG
    RE, PS = MG.reference_sample_methods()
    torch.set_num_threads(4)
    os.makedirs(out_dir, exist_ok=True)
    seen = {}                                     # (kind, class or planted column) -> events over the cases

    def run_reference(name, kind, mode, vox, fps, t0, opts, seed, ieee):
        plant = np.random.default_rng([CASES[name][6], seed])       # (the seed search moves the planted draws too)
        with MG.DrawCapture() as cap:
            true_rand = cap.rand0

            def planting_rand(*a, **k):           # both torch.rand and the Bernoulli draw of DrawCapture come through here
                r = true_rand(*a, **k)
                flat = r.view(-1).numpy()         # shares r's memory
                pick = plant.random(flat.size)
                if r.dim() == 2:                  # a Bernoulli plane [H, W]
                    flat[pick < 0.02] = 0
                else:
                    flat[pick < 0.01] = 0
                    flat[pick >= 0.99] = TOP
                return r
            cap.rand0 = planting_rand
            try:
                torch.manual_seed(seed)
                y = torch.from_numpy(vox.copy())
                fn = (lambda: RE.sample_voxel_baseline(y, t0=t0, fps=fps, even=mode == "even", random=mode == "random")) \
                    if kind == "baseline" else (lambda: PS.sample_voxel_statistical(y, t0=t0, fps=fps, **opts))
                if ieee:
                    with MG.IeeeSqrt():
                        res = fn()
                else:
                    res = fn()
            finally:
                cap.rand0 = true_rand
        return [np.asarray(r) for r in res], cap

    for name, (kind, mode, shape, fps, t0, opts, grid_seed) in CASES.items():
        OS.offsets(fps, t0)                       # raises unless the reference's arange has 10 elements at this fps
        vox, at = edge_voxels(np.random.default_rng(grid_seed), shape)
        assert vox.dtype == F and np.isfinite(vox).all() and (vox >= 0).all()
        B, _, _, H, W = shape
        if name in POOLED:
            seed = 400
            res, cap = run_reference(name, kind, mode, vox, fps, t0, opts, seed, True)
        else:
            for seed in range(300, 360):
                res, cap = run_reference(name, kind, mode, vox, fps, t0, opts, seed, False)
                res_ieee, _ = run_reference(name, kind, mode, vox, fps, t0, opts, seed, True)
                if all(MG.events_equal(a, b) for a, b in zip(res, res_ieee)):
                    break
            else:
                raise AssertionError(f"{name}: MKL-VML sqrt and IEEE sqrt disagree for every seed tried")
        # the Bernoulli draws arrive plane by plane in pick_and_sort's order: frame, bin, negative (P index 1) first
        u_bern = np.empty((B, 2, 10, H, W), F)
        it = iter(cap.berns)
        for b in range(B):
            for c in range(10):
                for pi in (1, 0):
                    u_bern[b, pi, c] = next(it).numpy()
        rands = [r.numpy() for r in cap.rands]
        if mode == "even":
            assert not rands
            u_int, u_dec = np.zeros((B, 2, 10, H, W, 0), F), np.zeros((B, 2, 10, H, W), F)
        elif kind == "baseline":
            u_int, u_dec = rands[0].reshape(B, 2, 10, H, W, -1), rands[1].reshape(B, 2, 10, H, W)
        else:
            u_dec, u_int = rands[0].reshape(B, 2, 10, H, W), rands[1].reshape(B, 2, 10, H, W, -1)
        per_voxel, n, sel, used = voxel_events(vox, kind, mode, fps, t0, opts, u_int, u_dec, u_bern)
        if mode != "even":
            assert u_int.shape[-1] == int(n.max())
            u_int = np.where(np.arange(u_int.shape[-1]) < n[..., None], u_int, F(0)).astype(F)

        mine = run_oracle(vox, kind, mode, fps, t0, opts, u_int, u_dec, u_bern)
        if name in POOLED:
            diffs = [OS.events_close(a, np.asarray(b)) for a, b in zip(res, mine)]
            assert all(d >= 0 for d in diffs), (name, diffs)
        else:
            diffs = None
            assert all(MG.events_equal(a, b) for a, b in zip(res, mine)), name
        lens = np.array([len(r) for r in res], np.int64)
        assert per_voxel.sum(axis=(1, 2, 3, 4)).tolist() == lens.tolist()

        eff = effective(vox, kind)
        masks = classes(eff)
        class_voxels = np.array([int(masks[k].sum()) for k in CLASSES], np.int64)
        class_events = np.array([int(per_voxel[masks[k]].sum()) for k in CLASSES], np.int64)
        planted_events = np.array([int(per_voxel[b, pi, :, h, w].sum()) for b, pi, h, w in at], np.int64)
        assert class_voxels.min() > 0, (name, class_voxels)
        assert class_events[CLASSES.index("zero")] == 0
        integer = eff == np.rint(eff)
        assert not sel[integer].any()
        facts = {"bern0_on_integer": ((u_bern == 0) & integer).sum(), "u0_used": (used == 0).sum(), "utop_used": (used == TOP).sum()}
        if kind == "pure_slope":
            assert not per_voxel[:, :, 9].any()
        for k, e in list(zip(CLASSES, class_events)) + list(zip(PLANTED, planted_events)) + list(facts.items()):
            seen[kind, k] = seen.get((kind, k), 0) + int(e)

        ev = np.concatenate(res)
        assert ev.dtype.itemsize == 13
        path = os.path.join(out_dir, f"sampler_edges_{name}.npz")
        np.savez_compressed(path, vox=vox, kind=np.array(kind), mode=np.array(mode), fps=np.float64(fps), t0=np.float64(t0),
                            u_int=u_int, u_dec=u_dec, u_bern=u_bern, lens=lens, events=np.frombuffer(ev.tobytes(), np.uint8),
                            pooling_type=np.array(opts.get("pooling_type", "none")),
                            pooling_kernel_size=np.array(int(opts.get("pooling_kernel_size", 3))),
                            class_names=np.array(CLASSES), class_voxels=class_voxels, class_events=class_events,
                            planted_names=np.array(PLANTED), planted_at=at, planted_events=planted_events)
        assert os.path.getsize(path) <= MAX_BYTES, (path, os.path.getsize(path))
        print(f"{name}: torch seed {seed} shape={shape} fps={fps} t0={t0} M={u_int.shape[-1]} events={lens.tolist()} "
              f"bytes={os.path.getsize(path)} classes={dict(zip(CLASSES, class_events.tolist()))} "
              f"planted={dict(zip(PLANTED, planted_events.tolist()))} {({k: int(v) for k, v in facts.items()})}"
              + ("" if diffs is None else f" timestamps differing from the oracle by 1 us: {diffs}"))
    for kind in ("baseline", "pure_slope"):
        for k in CLASSES + PLANTED:
            assert (seen[kind, k] == 0) == (k == "zero"), (kind, k, seen[kind, k])
        # a planted Bernoulli draw of 0 on an exact integer; planted time draws of 0 and of 1 - 2^-24 behind emitted events
        assert seen[kind, "bern0_on_integer"] > 0 and seen[kind, "u0_used"] > 0 and seen[kind, "utop_used"] > 0, kind


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", ".sampler_edges"))
