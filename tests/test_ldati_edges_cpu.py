"""The C oracle on voxel values at the branch points of the relocation recurrence (exact integers, integer +- 1e-6, values
below 1e-6, -0.0, the float below an integer, a subnormal, negative values, counts beyond the slope table) against the
REFERENCE's own events for them (tests/golden/.ldati_edges, made by tests/make_ldati_edge_goldens.py), byte for byte.

A restatement of the recurrence with the 1e-6 dropped passes every other small fixture of this suite; it fails on each of
these."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ldati as O
from tests.make_ldati_edge_goldens import assert_classes
from tests.test_oracle_goldens_recipe import _compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", ".ldati_edges")
REF = os.environ.get("V2CE_REFERENCE_ROOT", "/root/reference")
CASES = ["slope", "slope_signed", "bidir", "bidir_signed", "none", "weighted_signed", "fps60_t0", "int16"]
SIGNED = {"slope": False, "slope_signed": True, "bidir": False, "bidir_signed": True, "none": False,
          "weighted_signed": True, "fps60_t0": True}


def load_case(name):
    """-> (vox as stored, uniforms, fps, t0, strategy, options, reference events, reference events per frame)"""
    z = np.load(os.path.join(GOLD, f"ldati_edges_{name}.npz"))
    opts = dict(bidirectional=bool(z["bidirectional"]), pooling_type=str(z["pooling_type"]),
                pooling_kernel_size=int(z["pooling_kernel_size"]))
    ref = np.frombuffer(z["events"].tobytes(), O.EVENT_DTYPE)
    return z["vox"], z["uniforms"], float(z["fps"]), float(z["t0"]), str(z["strategy"]), opts, ref, z["lens"]


def test_goldens_present():
    files = sorted(glob.glob(os.path.join(GOLD, "ldati_edges_*.npz")))
    assert [os.path.basename(f)[12:-4] for f in files] == sorted(CASES)
    for f in files:
        assert os.path.getsize(f) <= 250 * 1024, f


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference(name):
    vox, u, fps, t0, strategy, opts, ref, lens = load_case(name)
    seg, ts, x, y, p = O.emit_soa(vox, fps=fps, t0=t0, uniforms=u, strategy=strategy, **opts)
    assert np.array_equal(seg.sum(axis=1), lens)
    assert np.array_equal(ts, ref["timestamp"])
    mine = np.asarray(O.pack(ts, x, y, p))
    assert O.canonicalize(mine, seg.reshape(-1)).tobytes() == O.canonicalize(ref, seg.reshape(-1)).tobytes()


@pytest.mark.parametrize("name", CASES)
def test_classes_present(name):
    vox = load_case(name)[0]
    if name == "int16":
        assert vox.dtype == np.int16 and vox.min() == 0 and vox.max() == 9
        return
    assert vox.dtype == np.float32 and np.isfinite(vox).all()
    assert_classes(vox, SIGNED[name], name)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "scripts", "LDATI.py")), reason="the reference tree is not on this machine")
def test_recipe_regenerates_fixtures(tmp_path):
    out = tmp_path / ".ldati_edges"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "make_ldati_edge_goldens.py"), str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    made = sorted(os.listdir(out))
    assert made == sorted(os.listdir(GOLD)) == sorted(f"ldati_edges_{c}.npz" for c in CASES)
    _compare(str(tmp_path), [os.path.join(".ldati_edges", f) for f in made])
