"""What the tests of v2ce_convc_wgrad / v2ce_convc_dgrad (include/v2ce_hip_convcgrad.h) share: the channel pairs and the
shapes each of them runs.  The restatement of the header's formulas, the f64 truths, the seeded inputs, the share counts and
the bounds are those of tests/convn_ref.py and tests/grad_walk_ref.py, which do not fix the channel counts."""
from tests import convn_ref as N
from tests.convn_ref import (CAP, GROUP, PRIME_GRID, SMALL, WALK, dgrad_bound, dgrad_np, dgrad_shares, dgrad_truth,  # noqa: F401
                             inputs, pairs_of, to_c16_np, wgrad_bound, wgrad_np, wgrad_shares, wgrad_truth)

CHANNELS = (32, 64, 128, 256, 512)
# (cin, cout).  PAIRS run every shape of SMALL, (128, 128) the walk shape too; the asymmetric ones catch a transposed or
# truncated group index
PAIRS = ((128, 128), (128, 64), (64, 128), (32, 128))
WALK_PAIR = (128, 128)
# WIDE run three shapes only; 512 catches anything sized for four groups
WIDE = ((256, 256), (512, 512), (512, 32), (32, 512))
WIDE_SHAPES = ((2, 3, 5, 7), (1, 2, 3, 70), (1, 3, 20, 70))
# the widest pairs on the walk shape (396 tiles).  (256, 256) has 64 pairs: the default grid is 4 shares of 99 tiles, three
# flushes of the f32 chain and three tiles more, and the prime grid (97 // 64) one share; (512, 512) has 256 pairs: one share
# of 396 tiles and twelve flushes by default, on the largest workspace there is
LONG_WALKS = ((256, 256, WALK, 0), (256, 256, WALK, None), (512, 512, WALK, 0))
# where the older entries give the same bytes
NARROW = ((32, 32), (64, 64), (64, 32), (32, 64))
NARROW_SHAPES = ((1, 3, 20, 70), WALK)

assert all(s in SMALL for s in WIDE_SHAPES) and SMALL[(1, 3, 20, 70)] == 1 and N.WALK is WALK


def runs():
    """-> [(cin, cout, shape, mult)]: mult is max_workgroups as a multiple of the pair count (0: the default grid), None:
    the prime grid."""
    out = [(ci, co, shape, mult) for ci, co in PAIRS for shape, mult in SMALL.items()]
    out += [(*WALK_PAIR, WALK, 0), (*WALK_PAIR, WALK, None)]
    out += [(ci, co, shape, SMALL[shape]) for ci, co in WIDE for shape in WIDE_SHAPES]
    return out + list(LONG_WALKS)


def run_id(run):
    ci, co, shape, mult = run
    return f"{ci}to{co}_" + "x".join(map(str, shape)) + ("" if mult == 0 else "_one_share" if mult else "_grid97")


def cap_of(cin, cout, mult):
    return PRIME_GRID if mult is None else mult * pairs_of(cin, cout)
