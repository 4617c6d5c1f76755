"""INTEGRATION.md's list of V2CE_* environment switches against what the package reads: every variable that
v2ce-toolbox_amd/ reads is documented, no variable of the "Removed:" paragraph is read any more, and every variable of the
"Diagnostics" paragraph is still read."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ = re.compile(r'(?:getenv\(|os\.environ\.get\(|os\.environ\[)\s*"(V2CE_[A-Z0-9_]+)"')
NAME = re.compile(r"V2CE_[A-Z0-9_]+")


def _sources():
    for base, _, files in os.walk(os.path.join(ROOT, "v2ce-toolbox_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                with open(os.path.join(base, f), encoding="utf-8") as fh:
                    yield fh.read()


def _doc():
    """(names outside the "Removed:" paragraph, names inside it)"""
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        paragraphs = fh.read().split("\n\n")
    removed = [p for p in paragraphs if p.startswith("Removed:")]
    assert len(removed) == 1
    live = {n for p in paragraphs if p is not removed[0] for n in NAME.findall(p)}
    return live, set(NAME.findall(removed[0]))


def test_switches_read_are_documented_and_removed_ones_are_gone():
    read = {n for text in _sources() for n in READ.findall(text)}
    live, removed = _doc()
    assert len(read) > 20 and len(removed) >= 13, (len(read), len(removed))
    prefixes = tuple(n for n in live if n.endswith("_"))          # V2CE_BOX_<Ho>x<Wo>_..., V2CE_UPBOX_<H>x<W>_<n>
    undocumented = sorted(n for n in read if n not in live and not n.startswith(prefixes))
    assert not undocumented, f"read under v2ce-toolbox_amd/ but not in INTEGRATION.md: {undocumented}"
    assert not read & removed, f'in INTEGRATION.md\'s "Removed:" paragraph but still read: {sorted(read & removed)}'


def test_documented_diagnostics_are_still_read():
    texts = list(_sources())
    read = {n for text in texts for n in READ.findall(text)}
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        diagnostics = [p for p in fh.read().split("\n\n") if p.startswith("Diagnostics")]
    assert len(diagnostics) == 1
    names = set(NAME.findall(diagnostics[0]))
    assert len(names) > 20, len(names)
    # a prefix pattern (V2CE_BOX_<Ho>x<Wo>_...) is read under a name built at run time: its prefix opens a string literal
    stale = sorted(n for n in names if n not in read and not (n.endswith("_") and any('"' + n in t for t in texts)))
    assert not stale, f'in INTEGRATION.md\'s "Diagnostics" paragraph but not read under v2ce-toolbox_amd/: {stale}'
