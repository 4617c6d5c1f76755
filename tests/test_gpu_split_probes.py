"""Every split-half conv instance of the default dispatch, bit for bit, on data where its arithmetic is exact.

tests/split_probe_ref.py builds the rows (one per row of test_gpu_tile_walk.WALK_CASES, at the smallest shape that keeps the
instance and at least two ragged boxes along H and W), the data of the probes and the f64 truth, and states the three
conditions under which a split-half launch must return the truth in every element; tests/test_split_probe_cpu.py proves
them for every row and probe and shows on a model which probe catches which fault.  Here, through the launcher of the tile
walks (the model's own entry points):

P1 - P3 (narrow x narrow, wide activations, wide weights; the pred rows run P3 twice: wp wide, then as P3w w wide), per row:
- the profile names exactly the row's instance;
- y (and y2, the fused shortcut) equals the f64 truth rounded to f32 -- the truth is an f32 except on the head's leaky side,
  which is one rounding of pre-activation x float32(0.01) -- compared as int32; a failure prints the mismatch pattern;
- the range slot's column 0 is max |y| exactly (not for the fused head, which materialises no y);
- each sequence launched alone returns the batch's bytes (the instance that ran, where it is not the row's, is printed);
- sequence 1 (2^8 x sequence 0) is 2^8 x the launch of sequence 0 with the shared shifts scaled down alike (rows of B = 2);
- the exact-f32 kernels (the launcher of tests/test_gpu_f32_conv.py; the kinds it can run: plain convs with or without a
  residual, upsample ++ skip, the head) return the same bytes on the same data.
Three rows run P1 at their full walk shape as well, across tile hand-overs.

P4: standard normals without additive terms, the same unit data at 2^-8, 1 and 2^8 (in launches of the row's own batch
size: the dispatch depends on it): every row is bitwise the unit row times its power of two, in y and y2."""
import time

import numpy as np
import pytest
import torch

import split_probe_ref as S
import test_gpu_f32_conv as F32
from test_gpu_grad_walks import describe_mismatch
from test_gpu_tile_walk import WALK_CASES, _sub, launch

pytestmark = pytest.mark.gpu

CASES = S.probe_cases()
FULL = [c for c in WALK_CASES if c.name in S.FULL_WALK_P1]
F32_KINDS = ("ws", "wt", "up", "up_sc", "head")


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def mismatch(got, want):
    return describe_mismatch(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want)))


def check_truth(c, probe, I):
    """The batched launch against the truth, in every element of every output; -> the launch's outputs."""
    got = launch(c, I)
    assert got["names"] == [c.name], got["names"]
    t = S.truth(c, I, "cuda")
    for key, t64 in t.items():
        want = t64.float()
        exact = torch.equal(want.double(), t64) if c.kind != "head" else torch.equal(want.double()[t64 >= 0], t64[t64 >= 0])
        assert exact and float(t64.abs().max()) > 0, (c.id, probe, key, "the truth is not an f32")
        want = want.cpu().numpy()
        assert got[key].shape == want.shape, (c.id, probe, key, got[key].shape, want.shape)
        assert same_bytes(got[key], want), (c.id, probe, key, mismatch(got[key], want))
    if c.kind != "pred":
        for b in range(I["k"].shape[0]):
            assert float(got["slot"][b, 0]) == float(np.abs(got["y"][b]).max()), (c.id, probe, b, got["slot"][b])
    return got


def f32_launch(c, I):
    """The same data through the exact-f32 kernels (planar tensors, the f32 test's launcher)."""
    Ho, Wo = c.out_hw
    B = I["k"].shape[0]
    up = c.kind.startswith("up")
    J = {"w": I["w"], "res": I.get("res", torch.zeros(B, c.Cout, c.T, Ho, Wo))}
    if c.kind == "head":
        J.update(x0=I["x"], scale=torch.ones(32), shift=I["bias"])
    else:
        J.update(x0=I["x0"], scale=I["scale"], shift=I["shift"])
    if up:
        J["x1"] = I["x1"]
    fc = F32.Case("f32", c.T, 2 if c.kind == "head" else c.C0, c.Cout, c.H, c.W, ks=c.ks, s=c.s, C1=c.C1,
                  src=((c.H + 1) // 2, (c.W + 1) // 2) if up else None, act=F32.LEAKY if c.kind == "head" else F32.RELU, B=B)
    return F32.launch(fc, J)["y"]


def run_probe(c, probe):
    t0 = time.time()
    I = S.inputs(c, probe)
    got = check_truth(c, probe, I)
    keys = [k for k in ("y", "y2") if got[k] is not None]
    B = I["k"].shape[0]
    alone_names = set()
    for b in range(B):
        alone = launch(c, _sub(I, b))
        assert len(alone["names"]) == 1, alone["names"]
        alone_names.add(alone["names"][0])              # (the dispatch counts rounds over B: may be a neighbouring instance)
        for key in keys:
            assert same_bytes(alone[key][0], got[key][b]), (c.id, probe, key, b, mismatch(alone[key][0], got[key][b]))
    if B == S.B_PROBE:
        unit = launch(c, S.inputs_p0_unit_shift(c, probe))
        for key in keys:
            want = unit[key][0] * np.float32(2.0 ** S.SEQ_EXP)
            assert same_bytes(got[key][1], want), (c.id, probe, key, "sequence 1 is not 2^8 x sequence 0", mismatch(got[key][1], want))
    if c.kind in F32_KINDS:
        y32 = f32_launch(c, I)
        assert same_bytes(y32, got["y"]), (c.id, probe, "exact-f32 kernels", mismatch(y32, got["y"]))
    n = sum(got[k].size for k in keys)
    other = sorted(alone_names - {c.name})
    print(f"PROBE {c.name} {probe} [B, T, H, W] = {[B, c.T, c.H, c.W]} C {c.C0}+{c.C1} -> {c.Cout}: {n} elements bit-exact "
          f"({time.time() - t0:.2f} s)" + (f"; the sequences alone ran {other}" if other else ""))


@pytest.mark.parametrize("case,probe", [(c, p) for c in CASES for p in S.probes_of(c)], ids=lambda v: v if isinstance(v, str) else v.id)
def test_probe_is_bit_exact(case, probe):
    run_probe(case, probe)


@pytest.mark.parametrize("case", FULL, ids=lambda c: c.id)
def test_p1_is_bit_exact_across_tile_handovers(case):
    """P1 at the row's full walk shape: >= 3 tiles per workgroup, the sequences at 1, 2^8, 1."""
    t0 = time.time()
    got = check_truth(case, "P1", S.inputs(case, "P1"))
    n = sum(got[k].size for k in ("y", "y2") if got[k] is not None)
    print(f"PROBE {case.name} P1 (walk shape) [B, T, H, W] = {[case.B, case.T, case.H, case.W]}: {n} elements bit-exact "
          f"({time.time() - t0:.2f} s)")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_p4_power_of_two_scaling_is_bitwise(case):
    """'The result does not depend on the scales': inexact data, the same unit sequence at 2^-8, 1, 2^8."""
    n = 0
    units = []
    for exps in S.p4_batches(case):
        got = launch(case, S.inputs_p4(case, exps))
        assert got["names"] == [case.name], got["names"]
        u = exps.index(0)
        for key in ("y", "y2"):
            if got[key] is None:
                continue
            unit = got[key][u]
            assert np.isfinite(unit).all() and np.abs(unit).max() > 0
            assert ((unit == 0) | (np.abs(unit) >= 2.0 ** -100)).all()
            for b, e in enumerate(exps):
                want = unit * np.float32(2.0 ** e)
                assert same_bytes(got[key][b], want), (case.id, key, f"row {b} is not 2^{e} x the unit row", mismatch(got[key][b], want))
            units.append((key, unit))
            n += got[key].size
    for key, unit in units:                       # the unit row is the same in every launch
        first = next(v for k, v in units if k == key)
        assert same_bytes(unit, first), (case.id, key, "the unit row depends on its neighbours' scale")
    print(f"PROBE {case.name} P4 [B, T, H, W] = {[case.B, case.T, case.H, case.W]}: {n} elements scale bitwise")
