"""The split-half probes without a GPU: the case table against the dispatchers' variant queries and box
choices, the three exactness conditions of tests/split_probe_ref.py for every row and probe on the f64 restatement of the
split-half evaluation, and four mutants of that restatement, each with the probe that sees it.

What the mutants show is which assertion of tests/test_gpu_split_probes.py::test_probe_is_bit_exact fails on a kernel with
the same fault: the comparison of y with the f64 truth ("... elements differ"), on the probe named here.  P1 sees none of
them -- its lo halves are all zero and its values have three bits -- which is why P2 and P3 exist."""
import pytest
import torch

import split_probe_ref as S
from test_gpu_tile_walk import WALK_CASES, _variant

CASES = S.probe_cases()
PROBES = ("P1", "P2", "P3")
BY_NAME = {c.name: c for c in CASES}
WS_ROW = BY_NAME["conv3d_f16x2_ws_kernel<3,1,1,1,4,3,0,0,0>"]
WT_ROWS = [c for c in CASES if c.kind.startswith("wt")]


@pytest.mark.parametrize("case,walk", list(zip(CASES, WALK_CASES)), ids=lambda v: v.id if hasattr(v, "id") else None)
def test_probe_table(case, walk):
    """The row keeps the walk row's instance, kind and channels; the dispatcher still picks the instance at the probe's
    shape; whichever box the host side takes, H and W hold at least two boxes with ragged last ones."""
    for f in ("name", "kind", "ks", "s", "C0", "C1", "Cout", "tc", "res"):
        assert getattr(case, f) == getattr(walk, f), f
    assert _variant(case) == case.name
    assert case.H % 2 == 1 and case.W % 2 == 1
    if case.name in S.PROBE_HW:
        assert (case.B, case.T) == (S.B_PROBE, S.T_PROBE) and case.B * case.T * case.H * case.W < walk.B * walk.T * walk.H * walk.W
    else:                                     # the dispatcher gives the instance up at T = 3: the walk shape
        assert (case.B, case.T, case.H, case.W) == (walk.B, walk.T, walk.H, walk.W)
        for n in range(9, 121, 8):
            for hw in ((n, n), (n, n + 2), (n + 2, n)):
                small = S.Case(case.name, case.kind, S.B_PROBE, S.T_PROBE, case.C0, case.Cout, *hw, ks=case.ks, s=case.s, res=case.res,
                               C1=case.C1, tc=case.tc)
                assert _variant(small) != case.name, hw
    boxes = S.candidate_boxes(case)
    assert boxes and S.boxes_ok(case), boxes


def test_every_walk_instance_has_a_row():
    assert [c.name for c in CASES] == [c.name for c in WALK_CASES] and len({c.name for c in CASES}) == len(CASES)
    assert set(S.FULL_WALK_P1) <= set(BY_NAME) and set(S.PROBE_HW) <= set(BY_NAME)


def _is_f32(c, t64):
    """The truth is an f32 (the head's leaky side is one rounding of pre-activation x float32(0.01): only its other side)."""
    keep = t64 >= 0 if c.kind == "head" else torch.ones_like(t64, dtype=torch.bool)
    return torch.equal(t64.float().double()[keep], t64[keep])


@pytest.mark.parametrize("case,probe", [(c, p) for c in CASES for p in S.probes_of(c)], ids=lambda v: v if isinstance(v, str) else v.id)
def test_conditions_and_model(case, probe):
    I = S.inputs(case, probe)
    t = S.truth(case, I)
    m = S.model(case, I)
    cond = m["cond"]
    assert cond["a"], (case.id, probe, "(a): an operand is not hi + lo", cond["notes"][:3])
    assert cond["b"], (case.id, probe, "(b): a product has two non-zero lo halves")
    assert cond["c"], (case.id, probe, "(c): sum |w| |x| + |shift| + |res| reaches 2^24 units")
    for key, t64 in t.items():
        assert _is_f32(case, t64) and float(t64.abs().max()) < 2.0 ** 32, (case.id, probe, key)
        assert torch.equal(m[key], t64[0].float().double()), (case.id, probe, key, "the model is not the truth")
    wide = {"P1": (), "P2": S.ACT, "P3": S.WGT, "P3w": ("w",)}[probe]
    for name in wide:
        if name not in I or (case.kind == "pred" and probe == "P3" and name == "w"):
            continue
        v = I[name][0] if name in S.ACT else I[name]
        lo = S.split(v, S.pow2_prescale(float(v.abs().max())))[1]
        assert bool((lo != 0).all()), (case.id, probe, name, "an element of the wide side has a zero lo half")
    if probe == "P1":
        assert cond["lo_w"] == 0 and (cond["lo_x"] == 0 or case.kind == "pred")       # (pred: its intermediate y is wide)
        assert all(bool((I[n] != 0).all()) for n in S.WGT if n in I)
    if probe == "P2":
        assert cond["lo_w"] == 0 and cond["lo_x"] > 0
        for name in S.WGT:
            if name in I:
                w = I[name]
                assert bool((w != 0).any(dim=0).all()), (case.id, name, "a (tap, input channel) carries no weight")
                assert len({int(n) for n in (w != 0).reshape(w.shape[0], -1).sum(dim=1)}) == 1
    if probe == "P3w":                        # w wide, so the intermediate y is wide too; wp has no lo half
        assert cond["lo_w"] == int((S.split(I["w"], S.pow2_prescale(float(I["w"].abs().max())))[1] != 0).sum()) == I["w"].numel()
        assert cond["lo_x"] > 0 and cond["nonzero_sums"] >= 0.9, (case.id, cond)
    if probe == "P3":
        assert cond["lo_w"] > 0 and cond["lo_x"] == 0
        assert cond["nonzero_sums"] >= 0.95, (case.id, cond["nonzero_sums"])


def _differs(c, probe, mut):
    I = S.inputs(c, probe)
    plain, bad = S.model(c, I), S.model(c, I, mut)
    return float((plain["y"] != bad["y"]).double().mean())


def test_mutant_whxl_dropped_in_one_chunk():
    """w_h x_l skipped for the second 16-channel chunk: P2's truth comparison fails; P1 and P3 (x_l = 0) cannot see it."""
    mut = {"drop_whxl_chunk": 1}
    assert _differs(WS_ROW, "P2", mut) > 0.3
    assert _differs(WS_ROW, "P1", mut) == 0 and _differs(WS_ROW, "P3", mut) == 0


def test_mutant_wlxh_dropped_for_one_tap():
    """w_l x_h skipped for tap 13: P3's truth comparison fails; P1 and P2 (w_l = 0) cannot see it."""
    mut = {"drop_wlxh_tap": 13}
    assert _differs(WS_ROW, "P3", mut) > 0.05
    assert _differs(WS_ROW, "P1", mut) == 0 and _differs(WS_ROW, "P2", mut) == 0


def test_mutant_ten_bit_hi_half():
    """A hi plane of ten significant bits (lo formed against the 11-bit hi): P2 and P3 fail; P1's three-bit values pass."""
    mut = {"hi10": True}
    assert _differs(WS_ROW, "P2", mut) > 0.3 and _differs(WS_ROW, "P3", mut) > 0.3
    assert _differs(WS_ROW, "P1", mut) == 0


@pytest.mark.parametrize("case", WT_ROWS, ids=lambda c: c.id)
def test_mutant_g1_g2_swapped_in_the_lo_plane(case):
    """The lo plane of the Winograd-T weights built with G_1 and G_2 exchanged: P3 fails on every Winograd row; P1 and P2
    (integer and half-integer G_j of three bits: no lo half) cannot see it."""
    mut = {"swap_G12_lo": True}
    assert _differs(case, "P3", mut) > 0.3
    assert _differs(case, "P1", mut) == 0 and _differs(case, "P2", mut) == 0
