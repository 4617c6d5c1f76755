"""CPU: LDATI's size queries (plan, workspace, fused workspace, tile workspace, sweep LDS) answer every row of
tests/golden/.ldati_plan/plan_table.json with the integers recorded there -- the answers of the library before its host side was
rewritten around ldati_plan.h (tests/make_ldati_plan_table.py: the rows and the recipe)."""
import ctypes

from tests.make_ldati_plan_table import OUTPUTS, check_coverage, evaluate, load, prototypes, rows
from v2ce_toolbox_amd import hip


def test_table_holds_the_recipes_rows_on_both_sides_of_every_limit():
    table = load()
    inputs = [{k: v for k, v in r.items() if k not in OUTPUTS} for r in table]
    assert inputs == rows() and len(table) <= 2000
    check_coverage(table)


def test_size_queries_answer_as_recorded():
    hip.lib()                                         # (says how to build the library where it is missing)
    L = prototypes(ctypes.CDLL(hip.SO_PATH))          # a handle of its own: the prototypes of hip.lib() stay as they are
    wrong = []
    for r in load():
        got = evaluate(L, r)
        for c in OUTPUTS:
            if got[c] != r[c]:
                wrong.append(({k: v for k, v in r.items() if k not in OUTPUTS}, c, r[c], got[c]))
    assert not wrong, f"{len(wrong)} differences, the first: {wrong[:5]}"
