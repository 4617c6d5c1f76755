"""CPU side of the Dec1Conv layer tests (tests/test_gpu_dec1_conv_layer.py): the goldens of tests/golden/.dec1conv are
complete and small, their constants are stored once, and the numpy / torch f64 restatement the GPU test takes its sums of
|terms| from (tests/dec1_conv_ref.py) gives the reference's own gradients stored in them."""
import glob
import os

import numpy as np
import pytest

from tests import dec1_conv_ref as R
from tests import dec2_conv_ref as R2
from tests.last_conv_dgrad_ref import load_parts
from tests.make_last_block_dgrad_goldens import SIZE_CAP


def test_goldens_are_small_and_complete():
    files = sorted(glob.glob(os.path.join(R.GOLD, "*.npz")))
    assert len(files) >= 8 and all(os.path.getsize(p) <= SIZE_CAP == 300_000 for p in files)
    assert sum(os.path.getsize(p) for p in files) <= R.DIR_CAP == 9_000_000
    assert {os.path.basename(p).split(".")[0] for p in files} == set(R.CASES) | {R.SHARED}
    assert R.CASES is R2.CASES and len(R.CASES) == 2 and R.C == 128 and R.COLS == 3456
    # the constants are stored once: no case file holds one
    assert set(load_parts(os.path.join(R.GOLD, R.SHARED))) == set(R.CONSTS)
    for name, (B, L, H, W) in R.CASES.items():
        assert not set(load_parts(os.path.join(R.GOLD, name))) & set(R.CONSTS), name
        z = R.load_case(name)
        assert set(R.CONSTS) | {"t", "res", "upstream", "ref64_x0"} | {"ref64_" + k for k in R.GRADS} <= set(z), name
        for k in ("t", "res", "upstream"):
            assert z[k].shape == (B, R.C, L, H, W) and z[k].dtype == np.float32
        assert z["weight_bar"].shape == (R.C, R.C, 3, 3, 3) and z["ref64_d_weight_bar"].dtype == np.float64
        assert z["u"].shape == (R.C,) and z["v"].shape == (R.COLS,)
        assert (z["t"] == 0).mean() > 0.3 and z["t"].min() >= 0          # relu-like input


def test_the_maker_restates_dec2s_recipe_at_128_channels():
    """The goldens come from the reference's own modules; here: the maker's inputs are the stored ones (no reference tree is
    needed for them) and its constants the stored constants."""
    from tests import make_dec1_conv_goldens as M
    assert M.C == 128
    c = M.constants(71)
    z = load_parts(os.path.join(R.GOLD, R.SHARED))
    for k in R.CONSTS:
        assert np.array_equal(np.asarray(c[k]), z[k]), k
    for name in R.CASES:
        t, _, upstream = M.inputs(name)
        zc = load_parts(os.path.join(R.GOLD, name))
        assert np.array_equal(t, zc["t"]) and np.array_equal(upstream, zc["upstream"])      # (res is nudged off the kink)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_gives_the_references_gradients(name):
    z = R.load_case(name)
    c = {k: z[k] for k in R.CONSTS}
    g = R.layer_grads(c, z["t"], z["res"], z["upstream"])
    assert np.array_equal(g["pre"] > 0, z["ref64_x0"] > 0) and not (np.abs(g["pre"]) < 1e-4).any()
    assert 0.2 < (g["pre"] > 0).mean() < 0.8
    assert np.abs(g["x0"] - z["ref64_x0"]).max() <= 1e-11 * np.abs(z["ref64_x0"]).max()
    for k in R.GRADS:
        want = z["ref64_" + k]
        assert g[k].shape == want.shape and np.abs(want).max() > 0, k
        assert np.abs(g[k] - want).max() <= 1e-11 * np.abs(want).max(), (name, k)
    assert np.abs(g["u1"] - z["ref64_u_after"]).max() <= 1e-13 and np.abs(g["v1"] - z["ref64_v_after"]).max() <= 1e-13
    # d_res is the masked upstream, exactly
    assert np.array_equal(z["ref64_d_res"], np.where(z["ref64_x0"] > 0, z["upstream"].astype(np.float64), 0.0))
