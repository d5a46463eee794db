#!/usr/bin/env python3
"""The tables of profiles/rhs_edges/README.md from a log of the edge tests and the fixture.

    python -m pytest tests/test_rhs_edges.py -m gpu -q -rA > edges.log      # on the MI355X: the tests print every figure
    python tools/rhs_edges_table.py edges.log                               # -> markdown on stdout

Device figures are read from the lines test_rhs_edges.report() prints; the oracle's recorded errors from tests/golden/rhs_edges.npz.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(f64|f32) (rhs|g|dg|Gamma) (\w+?)(?: path (\d))? \| (.*)$")
CELL = re.compile(r"(\w+)\s+([0-9.e+-]+|nan|inf) \(bar ([0-9.e+-]+)\)")


def parse(path):
    """-> {(prec, quantity, variant, path or None): {family: (err, bar)}}"""
    out = {}
    for line in open(path, errors="replace"):
        m = LINE.match(line.strip())
        if m:
            out[(m.group(1), m.group(2), m.group(3), m.group(4))] = {c[0]: (float(c[1]), float(c[2])) for c in CELL.findall(m.group(5))}
    return out


def main(log):
    got = parse(log)
    f = np.load(os.path.join(ROOT, "tests", "golden", "rhs_edges.npz"))
    fams, variants = list(f["families"]), list(f["variants"])
    e = lambda v: "%.1e" % v
    print("| variant | family | oracle f64 | bar f64 | path 0 | path 1 | path 2 | f32 path 0 | f32 path 1 | f32 path 2 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for v in variants:
        orc = f[f"f64_{v}_ud_oracle_err"].max(axis=1)
        for i, fam in enumerate(fams):
            d64 = [got[("f64", "rhs", v, p)][fam] for p in "012"]
            d32 = [got[("f32", "rhs", v, p)][fam][0] for p in "012"]
            print(f"| {v} | {fam} | {e(orc[i])} | {e(d64[0][1])} | " + " | ".join(e(d[0]) for d in d64) + " | " + " | ".join(e(d) for d in d32) + " |")
    print()
    print("| variant | family | g: oracle / bar / f64 / f32 | ∂g: oracle / bar / f64 / f32 | Γ: oracle / bar / f64 / f32 |")
    print("|---|---|---|---|---|")
    for v in variants:
        orc = f[f"f64_{v}_tensor_oracle_err"].max(axis=1)
        for i, fam in enumerate(fams):
            cells = []
            for j, q in enumerate(("g", "dg", "Gamma")):
                d64, d32 = got[("f64", q, v, None)][fam], got[("f32", q, v, None)][fam]
                cells.append(f"{e(orc[i, j])} / {e(d64[1])} / {e(d64[0])} / {e(d32[0])}")
            print(f"| {v} | {fam} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main(sys.argv[1])
