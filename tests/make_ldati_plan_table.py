"""Recipe of tests/golden/.ldati_plan/plan_table.json: what LDATI's size queries answer on the limits the host code names.

All of them are pure host functions (no GPU): v2ce_ldati_plan_info (return code and its ten words), v2ce_ldati_workspace_bytes
(SoA and packed output), v2ce_ldati_fused_ws_bytes, v2ce_ldati_tile_ws_bytes and v2ce_ldati_lds_bytes.  The table was written
once by the library of the commit BEFORE the host side of csrc/ldati.hip was given one plan, one workspace layout and one path
choice (ldati_plan.h); tests/test_ldati_plan_table.py asks the present library the same questions and wants the same integers.

Rows (rows()): one family varied at a time around three base points -- 346x260 B=4, 1384x260 B=8, 64x32 B=1 -- on both sides of
every limit: tile counts (kMaxTiles), B*9 <= 65535, the key range against fps / t0, every option and the rejected ones, the
event counts where the sort workgroup, the tile workgroup and the LDS capacity change, the fused hints and the 2^30-slot
limit, and the per-call V2CE_LDATI_* switches (set through the process environment; the once-per-process ones stay unset).
Rows with strategy 'random' and events record plan_info only: their workspace holds rocPRIM's temporary size, which is not a
fact of this code.

    python tests/make_ldati_plan_table.py <path of libv2ce_hip.so> [out.json]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", ".ldati_plan", "plan_table.json")
SWITCHES = ("V2CE_LDATI_SORT_THREADS", "V2CE_LDATI_SPAN_KEYS", "V2CE_LDATI_NO_SPARSE", "V2CE_LDATI_NO_FUSED", "V2CE_LDATI_OLD_TILE")
ONCE = ("V2CE_LDATI_TILE_THREADS", "V2CE_LDATI_NB_SOFT", "V2CE_LDATI_DENSE_NW")
INPUTS = ("B", "H", "W", "fps", "t0", "options", "total", "max_segment", "max_tile", "segment_hint", "tile_bin_hint", "env")
OUTPUTS = ("rc", "info", "workspace_soa", "workspace_packed", "fused_ws", "tile_ws", "lds")
SLOPE, NONE, RANDOM = 0, 1, 2
POOL_NONE, POOL_AVG, POOL_WEIGHTED = 0, 1, 2

BASES = ((4, 260, 346), (8, 260, 1384), (1, 32, 64))
SHAPES = ((1, 1, 1), (1, 4, 4), (1, 32, 64), (1, 45, 46), (1, 724, 724), (1, 725, 725), (7281, 32, 64), (7282, 32, 64))
TIMES = ((30.0, 0.0), (10.0, 0.0), (60.0, 0.5), (240.0, 0.0), (30.0, 1000.0), (5.0, 0.0), (1.0, 0.0), (0.5, 0.0))
OPTIONS = ((None,) + tuple((s, b, POOL_NONE, 3) for s in (SLOPE, NONE, RANDOM) for b in (0, 1)) +
           ((SLOPE, 0, POOL_AVG, 3), (SLOPE, 0, POOL_AVG, 15), (SLOPE, 0, POOL_WEIGHTED, 3)) +
           ((7, 0, POOL_NONE, 3), (SLOPE, 0, POOL_AVG, 4), (SLOPE, 0, POOL_AVG, 17)))          # rejected
COUNTS = ((0, 0, 0), (100, 50, 10), (10 ** 5, 2 * 10 ** 4, 500), (10 ** 6, 85000, 3000),
          (10 ** 5, 2048, 500), (10 ** 5, 2049, 500), (10 ** 5, 2 * 10 ** 4, 4096), (10 ** 5, 2 * 10 ** 4, 4097),
          (10 ** 6, 85000, 15360), (10 ** 6, 85000, 15361), (2 ** 32 - 1, 85000, 3000), (2 ** 32, 85000, 3000))
SEGMENT_HINTS = (0, 2048, 2049, 85000, 1400000)
TILE_BIN_HINTS = (0, 256, 5000, 15360, 15361)
ENVS = tuple({"V2CE_LDATI_SORT_THREADS": v} for v in ("64", "128", "256", "7")) + \
       tuple({"V2CE_LDATI_SPAN_KEYS": v} for v in ("128", "256", "512")) + \
       ({"V2CE_LDATI_NO_SPARSE": "1"}, {"V2CE_LDATI_NO_FUSED": "1"}, {"V2CE_LDATI_OLD_TILE": "1"})
DEFAULT = dict(fps=30.0, t0=0.0, options=None, total=10 ** 5, max_segment=2 * 10 ** 4, max_tile=500, segment_hint=2 * 10 ** 4,
               tile_bin_hint=0, env={})


def rows():
    out = []

    def add(shape, **changes):
        r = dict(DEFAULT, B=shape[0], H=shape[1], W=shape[2])
        r.update(changes)
        r["options"] = list(r["options"]) if r["options"] is not None else None
        if r not in out:
            out.append(r)

    bidir, random, none = (SLOPE, 1, POOL_NONE, 3), (RANDOM, 0, POOL_NONE, 3), (NONE, 0, POOL_NONE, 3)
    for shape in SHAPES:
        add(shape)
        add(shape, tile_bin_hint=5000)
        add(shape, options=random)
    for i, base in enumerate(BASES):                       # the other options ride on the first base point only
        for fps, t0 in TIMES:
            for o in (None, bidir, random)[:3 if i == 0 else 1]:
                add(base, fps=fps, t0=t0, options=o)
        for o in OPTIONS:
            add(base, options=o)
            if i == 0:
                add(base, options=o, tile_bin_hint=5000)
        for total, seg, tile in COUNTS:
            for o in (None, bidir, random)[:3 if i == 0 else 1]:
                add(base, options=o, total=total, max_segment=seg, max_tile=tile)
        for sh in SEGMENT_HINTS:
            for th in TILE_BIN_HINTS:
                for o in (None, bidir, none)[:3 if i == 0 else 1]:
                    add(base, options=o, segment_hint=sh, tile_bin_hint=th)
        for env in ENVS:
            for th in (0, 5000)[:2 if i == 0 else 1]:
                add(base, total=10 ** 6, max_segment=85000, max_tile=3000, segment_hint=85000, tile_bin_hint=th, env=dict(env))
    for B in (64, 96):                       # either side of 2^30 record slots
        add((B, 260, 346), segment_hint=85000, tile_bin_hint=15360)
    return out


class _Options(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("strategy", "bidirectional", "pooling_type", "pooling_kernel_size")]


def prototypes(L):
    i32, i64, f64, sz, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
    L.v2ce_ldati_plan_info.argtypes, L.v2ce_ldati_plan_info.restype = [i32, i32, i32, f64, f64, vp, i64, i64, i64, vp], ctypes.c_int
    L.v2ce_ldati_workspace_bytes.argtypes, L.v2ce_ldati_workspace_bytes.restype = [i32, i32, i32, f64, f64, vp, i64, i64, i64, i32], sz
    L.v2ce_ldati_fused_ws_bytes.argtypes, L.v2ce_ldati_fused_ws_bytes.restype = [i32, i32, i32, f64, f64, vp, i64, i64], sz
    L.v2ce_ldati_tile_ws_bytes.argtypes, L.v2ce_ldati_tile_ws_bytes.restype = [i32, i32, i32], sz
    L.v2ce_ldati_lds_bytes.argtypes, L.v2ce_ldati_lds_bytes.restype = [f64, f64], sz
    return L


def evaluate(L, r):
    """The OUTPUTS of one row from library L (prototypes set), with exactly the row's switches in the environment."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES + ONCE}
    os.environ.update(r["env"])
    try:
        o = _Options(*r["options"]) if r["options"] is not None else None
        op = ctypes.cast(ctypes.byref(o), ctypes.c_void_p) if o is not None else None
        geometry = (r["B"], r["H"], r["W"], r["fps"], r["t0"], op)
        counts = (r["total"], r["max_segment"], r["max_tile"])
        info = (ctypes.c_int64 * 10)()
        res = {"rc": int(L.v2ce_ldati_plan_info(*geometry, *counts, ctypes.cast(info, ctypes.c_void_p))), "info": [int(v) for v in info]}
        if r["options"] is not None and r["options"][0] == RANDOM and r["total"] > 0:
            return dict(res, workspace_soa=None, workspace_packed=None, fused_ws=None, tile_ws=None, lds=None)
        res["workspace_soa"] = int(L.v2ce_ldati_workspace_bytes(*geometry, *counts, 0))
        res["workspace_packed"] = int(L.v2ce_ldati_workspace_bytes(*geometry, *counts, 1))
        res["fused_ws"] = int(L.v2ce_ldati_fused_ws_bytes(*geometry, r["segment_hint"], r["tile_bin_hint"]))
        res["tile_ws"] = int(L.v2ce_ldati_tile_ws_bytes(r["B"], r["H"], r["W"]))
        res["lds"] = int(L.v2ce_ldati_lds_bytes(r["fps"], r["t0"]))
        return res
    finally:
        for k in r["env"]:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def coverage(table):
    """Both outcomes of every limit the rows sit on, as {name: set of outcomes seen}."""
    seen = {k: set() for k in ("rc", "ok", "fused", "workspace", "lds", "sort_threads", "tile_threads", "sort_records_per_thread")}
    for r in table:
        ok, shift, NB, T, capA, cap2, n_tab, n_bkt, lds_tile, lds_sort = r["info"]
        seen["rc"].add(r["rc"])
        if r["rc"]:
            continue
        seen["ok"].add(ok)
        big = r["max_segment"] > 2048
        seen["sort_records_per_thread"].add(24 if big else 8)
        if big:
            seen["sort_threads"].add(cap2 // 24)
        # lds_tile = (2 capA + 2048) 4 + 2048 * 8 + (threads / 128) NB 4 + 2 (threads / 64 + 1) 4
        rest = lds_tile - (2 * capA + 2048) * 4 - 2048 * 8
        seen["tile_threads"].add({4 * NB * 4 + 72: 512, 8 * NB * 4 + 136: 1024}[rest])
        if r["fused_ws"] is not None:
            seen["fused"].add((r["tile_bin_hint"] > 0, r["fused_ws"] > 0))
            seen["workspace"].add(r["workspace_packed"] > 0)
            seen["lds"].add(r["lds"] > 0)
    return seen


def check_coverage(table):
    seen = coverage(table)
    assert seen["rc"] == {0, -1, -2}, seen["rc"]
    assert seen["ok"] == {0, 1} and seen["workspace"] == {False, True} and seen["lds"] == {False, True}, seen
    assert seen["fused"] == {(d, nz) for d in (False, True) for nz in (False, True)}, seen["fused"]
    assert seen["sort_threads"] == {64, 128, 256} and seen["tile_threads"] == {512, 1024}, seen
    assert seen["sort_records_per_thread"] == {8, 24}, seen
    return seen


def main(argv):
    L = prototypes(ctypes.CDLL(os.path.abspath(argv[1])))
    out = argv[2] if len(argv) > 2 else TABLE
    table = [dict(r, **evaluate(L, r)) for r in rows()]
    assert len(table) <= 2000, len(table)
    for name, outcomes in check_coverage(table).items():
        print(f"{name}: {sorted(outcomes, key=str)}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w", encoding="utf-8") as fh:
        fh.write('{"columns": %s,\n "rows": [\n' % json.dumps(list(INPUTS + OUTPUTS)))
        fh.write(",\n".join("  " + json.dumps([r[c] for c in INPUTS + OUTPUTS]) for r in table))
        fh.write("\n]}\n")
    print(f"{len(table)} rows -> {out} ({os.path.getsize(out)} bytes)")


def load(path=TABLE):
    with open(path, encoding="utf-8") as fh:
        doc = json.load(fh)
    return [dict(zip(doc["columns"], row)) for row in doc["rows"]]


if __name__ == "__main__":
    main(sys.argv)
