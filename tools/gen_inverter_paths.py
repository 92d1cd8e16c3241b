#!/usr/bin/env python3
"""Generates tests/golden/inverter_paths.json: operands of the division-step inverter (csrc/h2v_modinv.hpp) sorted by the
way they leave it.  A seeded search with the integer model of tests/safegcd_model.py: DRAWS uniform operands per field, each
classified as (sign of f at exit, +M repairs, final -M taken, batches); per class the first KEEP operands met are stored - all
of them where a class turns up fewer times - together with how often the class was met.  Numbers and class labels only.

A few minutes of plain Python; no test runs it.  tests/test_inverter_paths.py checks every stored operand against its label
and that the classes of safegcd_model.RARE / RARE_BATCHES are all there.

    python tools/gen_inverter_paths.py            # writes the fixture, prints the class table of DESIGN.md 4.5
"""
import collections
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import safegcd_model as S  # noqa: E402

DRAWS = 25000
KEEP = 8
SEEDS = {"FP": 11, "FR": 12}


def search(name):
    fld = S.field(name)
    rng = random.Random(SEEDS[name])
    counts, kept = collections.Counter(), collections.defaultdict(list)
    zlo = zhi = -1
    for _ in range(DRAWS):
        x = rng.randrange(1, fld.mod)
        inv, cls, (lo, hi) = S.inverse(x, fld)
        assert inv * x % fld.mod == 1
        zlo, zhi = min(zlo, lo), max(zhi, hi)
        lab = S.label(cls)
        counts[lab] += 1
        if len(kept[lab]) < KEEP:
            kept[lab].append("%x" % x)
    return {"seed": SEEDS[name], "draws": DRAWS, "zeta_range": [zlo, zhi], "counts": dict(sorted(counts.items())),
            "classes": dict(sorted(kept.items()))}


def table(name, doc):
    cls = {S.parse_label(lab): n for lab, n in doc["counts"].items()}
    rows = [(what, sum(n for c, n in cls.items() if pick(c))) for what, pick in S.RARE.items()]
    rows += [("%d batches" % b, sum(n for c, n in cls.items() if c[3] == b)) for b in S.RARE_BATCHES[name] + (S.COMMON_BATCHES[name],)]
    return rows


def main():
    doc = {name: search(name) for name in ("FP", "FR")}
    with open(S.FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for name in ("FP", "FR"):
        print(name, "of", DRAWS, "zeta", doc[name]["zeta_range"])
        for what, n in table(name, doc[name]):
            print("  %-22s %6d" % (what, n))
        for lab, n in doc[name]["counts"].items():
            print("    %-40s %6d  kept %d" % (lab, n, len(doc[name]["classes"][lab])))


if __name__ == "__main__":
    main()
