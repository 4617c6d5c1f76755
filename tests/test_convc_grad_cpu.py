"""CPU side of the tests of v2ce_convc_wgrad / v2ce_convc_dgrad (include/v2ce_hip_convcgrad.h, tests/test_gpu_convcgrad.py):
the header's symbols, the size queries of all 25 channel pairs and of what is refused, the refusals on never-dereferenced
addresses at 128 -> 128, the workspace formulas and the share arithmetic up to 16 x 16 pairs, the exactness margins of the
integer data of check A, and the f64 truth against the numpy restatement at an asymmetric wide pair."""
import glob
import os
import re

import numpy as np
import pytest

from tests import convc_ref as R
from tests import grad_walk_ref as G
from v2ce_toolbox_amd import conv_grads, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "v2ce_hip_convcgrad.h"
BAD_ARG, WORKSPACE = -1, -4
PARTIAL = (27 * 32 * 32 + 32) * 8                                    # f64 bytes of one workgroup's partial sums
ALL = tuple((ci, co) for ci in R.CHANNELS for co in R.CHANNELS)
REFUSED = ((0, 32), (16, 32), (96, 128), (128, 96), (1024, 32), (32, 1024), (-128, 128), (160, 160))


def entries():
    L = hip.lib()
    return ((L.v2ce_convc_wgrad_workspace_bytes, L.v2ce_convc_wgrad, "x"),
            (L.v2ce_convc_dgrad_workspace_bytes, L.v2ce_convc_dgrad, "weight"))


def test_library_exports_exactly_the_symbols_of_the_convcgrad_header():
    L = hip.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(v2ce_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 4 and set(syms) == set(hip.CONVCGRAD_EXPORTS) and len(set(hip.CONVCGRAD_EXPORTS)) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert hip.CONVC_CHANNELS == R.CHANNELS and hip.CONVN_CHANNELS == (32, 64)
    for other in (hip.EXPORTS, hip.GRAD_EXPORTS, hip.TRAIN_EXPORTS, hip.CONVGRAD_EXPORTS, hip.CONVDGRAD_EXPORTS,
                  hip.CONVUPGRAD_EXPORTS, hip.CONVUPDGRAD_EXPORTS, hip.CONVNGRAD_EXPORTS, hip.CONVUPNGRAD_EXPORTS,
                  hip.CONVUPNDGRAD_EXPORTS):
        assert not set(hip.CONVCGRAD_EXPORTS) & set(other)
    for other in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(other) != HEADER:
            assert not any(s in open(other).read() for s in syms), other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "hip.CONVCGRAD_EXPORTS" in entry
    assert conv_grads._CONVC_WGRAD == ("v2ce_convc_wgrad", (R.CHANNELS, R.CHANNELS), True)
    assert conv_grads._CONVC_DGRAD == ("v2ce_convc_dgrad", (R.CHANNELS, R.CHANNELS), True)


def test_size_queries_of_every_pair_and_of_what_is_refused():
    d = (2, 3, 5, 7, 7)
    assert len(ALL) == 25
    for q, _, _ in entries():
        for cin, cout in ALL:
            assert q(cin, cout, *d, 0) > 0, (cin, cout)
        for cin, cout in REFUSED:
            assert q(cin, cout, *d, 0) == 0, (cin, cout)
    # the older entries keep their channel set
    L = hip.lib()
    for q in (L.v2ce_convn_wgrad_workspace_bytes, L.v2ce_convn_dgrad_workspace_bytes):
        for cin, cout in ALL:
            assert (q(cin, cout, *d, 0) > 0) == (cin <= 64 and cout <= 64), (cin, cout)


def test_refusals_without_gpu():
    L = hip.lib()
    a, big = 4096, 1 << 30                                              # aligned stand-ins for device addresses
    d = (2, 3, 5, 7, 7)
    ok = (128, 128)
    for q, f, first in entries():
        for cin, cout in REFUSED:
            assert f(a, a, a, cin, cout, *d, a, a, a, big, 0, None) == BAD_ARG
            assert b"cin" in L.v2ce_last_error() and b"512" in L.v2ce_last_error()
        assert q(*ok, 0, 3, 5, 7, 7, 0) == 0 and q(*ok, 2, 0, 5, 7, 7, 0) == 0 and q(*ok, 2, 3, 0, 7, 7, 0) == 0
        assert q(*ok, 2, 3, 5, 0, 7, 0) == 0 and q(*ok, 2, 3, 5, 7, 6, 0) == 0 and q(*ok, *d, -1) == 0
        assert q(*ok, 4096, 4096, 16, 16, 16, 0) == 0                    # 2^32 positions
        assert q(*ok, 1, 1 << 20, 1, 1 << 10, 1 << 14, 0) == 0           # B L H pitch = 2^34
        # refused before anything is launched (the addresses below are never dereferenced)
        assert f(a, a, a, *ok, 2, 3, 5, 7, 6, a, a, a, big, 0, None) == BAD_ARG       # pitch < W
        assert f(a, a, a, *ok, *d, a, a, a, big, -1, None) == BAD_ARG
        assert f(None, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, None, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, a, *ok, *d, a, a, None, big, 0, None) == BAD_ARG and b"null" in L.v2ce_last_error()
        assert f(a, a, a, *ok, *d, None, None, a, big, 0, None) == BAD_ARG and b"no output" in L.v2ce_last_error()
        assert f(a, a + 4, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # y
        assert f(a, a, a + 8, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # upstream
        assert f(a, a, a, *ok, *d, a, a, a + 4, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()      # workspace
        if first == "x":
            assert f(a + 4, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()
        else:
            assert f(a + 2, a, a, *ok, *d, a, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # weight
            assert f(a, a, a, *ok, *d, a + 4, a, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # d_x
            assert f(a, a, a, *ok, *d, a, a + 8, a, big, 0, None) == BAD_ARG and b"aligned" in L.v2ce_last_error()  # d_res
        need = q(*ok, *d, 0)
        rc = f(a, a, a, *ok, *d, a, a, a, need - 4, 0, None)
        assert rc == WORKSPACE and b"workspace too small" in L.v2ce_last_error()
        assert L.v2ce_last_error().startswith(b"v2ce_convc_")


def test_size_queries_follow_the_header_formulas():
    L = hip.lib()
    (qw, _, _), (qd, _, _) = entries()
    up256 = lambda n: (n + 255) // 256 * 256
    shapes = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 7), (1, 3, 20, 70, 96), (1, 16, 65, 87, 96), R.WALK + (G.pitch_of(R.WALK[3]),)]
    most = 0
    for cin, cout in ALL:
        p = R.pairs_of(cin, cout)
        assert 1 <= p <= 256 and R.CAP % p == 0
        for d in shapes:
            tiles = G.conv_tiles(*d[:4])
            for cap in (0, 1, 3, 16, 97, 255, 256, 257, 512, 1000):
                shares = R.wgrad_shares(cin, cout, tiles, cap)
                assert 1 <= shares and shares * p <= R.CAP, (cin, cout, d, cap)
                assert qw(cin, cout, *d, cap) == up256(shares * p * PARTIAL), (cin, cout, d, cap)
                assert qd(cin, cout, *d, cap) == up256(27 * cin * cout * 4)                      # the grid needs nothing
                assert 1 <= R.dgrad_shares(cin, tiles, cap) * (cin // 32) <= R.CAP
                most = max(most, qw(cin, cout, *d, cap))
        if cin <= 64 and cout <= 64:                                    # the sizes of the older entries
            assert all(qw(cin, cout, *d, c) == L.v2ce_convn_wgrad_workspace_bytes(cin, cout, *d, c) and
                       qd(cin, cout, *d, c) == L.v2ce_convn_dgrad_workspace_bytes(cin, cout, *d, c)
                       for d in shapes for c in (0, 3, 97, 300))
    assert most == 256 * PARTIAL and most < 57 * 10 ** 6                # the workspace is bounded: 56.7 MB
    # 16 x 16 pairs: one share whatever the tiles and the cap are
    assert R.pairs_of(512, 512) == 256
    for tiles in (1, 60, 396, 10 ** 6):
        for cap in (0, 1, 255, 256, 1000):
            assert R.wgrad_shares(512, 512, tiles, cap) == 1
    assert R.wgrad_shares(512, 256, 396, 0) == 2 and R.wgrad_shares(128, 128, 396, 0) == 16
    assert R.wgrad_shares(128, 128, 396, R.PRIME_GRID) == 6 and R.dgrad_shares(128, 396, R.PRIME_GRID) == 24
    assert R.dgrad_shares(512, 396, 0) == 16 and R.dgrad_shares(512, 396, 5) == 1
    # the one-share runs: 60 tiles, a full chain of 32 tiles and a partial one of 28
    assert G.conv_tiles(1, 3, 20, 70) == 60 and hip.WGRAD_CHAIN // 128 == 32
    for cin, cout in R.PAIRS + R.WIDE:
        assert R.wgrad_shares(cin, cout, 60, R.cap_of(cin, cout, 1)) == 1
        assert qw(cin, cout, 1, 3, 20, 70, 96, R.cap_of(cin, cout, 1)) == R.pairs_of(cin, cout) * PARTIAL


def test_integer_sums_of_check_a_are_exact_in_f32():
    """With values 1 .. 3 a product is at most 9.  Below 2^24 every integer is an f32, so an fmaf chain, a sum of such
    chains in f64, the one rounding of the store and the plain f32 additions of the input gradient are exact in any order."""
    top = G.INT_MAX ** 2
    assert top == 9 and 27 * 512 * 9 < 2 ** 24 and 27 * max(hip.CONVC_CHANNELS) * top < 2 ** 24       # d_x
    shapes = {shape for _, _, shape, _ in R.runs()} | set(R.NARROW_SHAPES)
    assert R.WALK in shapes and len(shapes) == 7
    for shape in shapes:
        n = int(np.prod(shape))
        assert n * top < 2 ** 24 and n * G.INT_MAX < 2 ** 24              # d_weight; d_shift
    assert hip.WGRAD_CHAIN * top < 2 ** 24                               # one f32 chain


def test_run_lists():
    runs = R.runs()
    assert len(runs) == len(set(runs)) == 4 * 6 + 2 + 4 * 3 + 3
    assert {(ci, co) for ci, co, _, _ in runs} == set(R.PAIRS + R.WIDE)
    assert all(ci in R.CHANNELS and co in R.CHANNELS for ci, co in R.PAIRS + R.WIDE + R.NARROW)
    assert all(max(ci, co) > 64 for ci, co in R.PAIRS + R.WIDE) and all(max(ci, co) <= 64 for ci, co in R.NARROW)
    assert len({R.run_id(r) for r in runs}) == len(runs)
    wide = [r for r in runs if (r[0], r[1]) in R.WIDE and r not in R.LONG_WALKS]
    assert {r[2] for r in wide} == set(R.WIDE_SHAPES)
    # the long walks of the widest pairs: shares of more than one chain at the default grid, up to twelve flushes
    tiles, chain = G.conv_tiles(*R.WALK), hip.WGRAD_CHAIN // 128
    assert runs[-3:] == list(R.LONG_WALKS) and tiles == 396 and chain == 32
    shares = [R.wgrad_shares(ci, co, tiles, R.cap_of(ci, co, m)) for ci, co, _, m in R.LONG_WALKS]
    assert shares == [4, 1, 1] and divmod(tiles // 4, chain) == (3, 3) and divmod(tiles, chain) == (12, 12)
    assert int(np.prod(R.WALK)) * G.INT_MAX ** 2 == 304182             # the largest integer sum of check A
    assert all(R.cap_of(ci, co, m) == R.pairs_of(ci, co) for ci, co, s, m in wide if s == (1, 3, 20, 70))


def test_truth_matches_the_numpy_restatement_at_128_to_64():
    """The f64 truth of the GPU tests (one matmul per tap) against the header's formulas term by term, where the two sides
    have different group counts: each is within n 2^-53 S of the exact sum of an element's n terms."""
    cin, cout, shape = 128, 64, (2, 3, 5, 7)
    z = R.inputs(shape, cin, cout, False, 17)
    tw, td = R.wgrad_truth(z["x"], z["y"], z["upstream"]), R.dgrad_truth(z["weight"], z["y"], z["upstream"])
    nw = R.wgrad_np(z["x"].numpy(), z["y"].numpy(), z["upstream"].numpy())
    nd = R.dgrad_np(z["weight"].numpy(), z["y"].numpy(), z["upstream"].numpy())
    n = max(int(np.prod(shape)), 27 * cout)
    assert tuple(tw["d_weight"].shape) == (cout, cin, 3, 3, 3) and tuple(td["d_x"].shape) == (2, cin, 3, 5, 7)
    assert np.all(np.abs(tw["d_weight"].numpy() - nw["d_weight"]) <= n * 2.0 ** -52 * tw["abs_weight"].numpy())
    assert np.all(np.abs(td["d_x"].numpy() - nd["d_x"]) <= n * 2.0 ** -52 * td["abs_x"].numpy())
    assert np.all(np.abs(tw["d_shift"].numpy() - nw["d_shift"]) <= n * 2.0 ** -52 * tw["abs_shift"].numpy())
    assert np.array_equal(td["d_res"].numpy(), nd["d_res"])
    assert tw["abs_weight"].max() > 0 and td["abs_x"].max() > 0 and (nd["d_res"] == 0).mean() > 0.3
