#!/usr/bin/env python3
"""How many points the frontier form's select leaves between its bound and the exact theta (tests/closure_bound_model.theta_bound
against closure_model.theta_of): every one of them that a traversal discovers is a single pop instead of a frontier member.  CPU only.

  scripts/closure_bound_gap.py [--n 31250] [--top 977] [--queries 64] [--ef 200 400]

Draws `n` rows and the queries from the bench's SiftLike generator (the upper points of the 1 M graph are a random 1/32 of the base, the
TOP set a random 1/32 of those) and prints, per ef and set, the key range in bits and the points in [bound, theta) per query."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from muopdb_amd import synth as S  # noqa: E402
from tests import closure_bound_model as BM  # noqa: E402
from tests import closure_model as CM  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=31250)
    p.add_argument("--top", type=int, default=977)
    p.add_argument("--queries", type=int, default=64)
    p.add_argument("--ef", type=int, nargs="+", default=[200, 400])
    p.add_argument("--json", default=None)
    a = p.parse_args()
    gen = S.SiftLike(128, seed=1, device="cpu")
    x = gen.draw(a.n, seed=11).numpy().astype(np.float32)
    q = gen.draw(a.queries, seed=1000).numpy().astype(np.float32)
    out = {}
    for ef in a.ef:
        for name, rows in (("all upper points", x), ("TOP set", x[:a.top])):
            gaps, bits = [], []
            for qi in range(len(q)):
                d = ((rows - q[qi]) ** 2).sum(1, dtype=np.float32)
                keys = BM.images(d)
                tb, th = BM.theta_bound(keys, ef), CM.theta_of(keys, ef)
                gaps.append(sum(1 for v in keys if tb <= v < th))
                bits.append((max(keys) - min(keys)).bit_length())
            out["ef %d, %s" % (ef, name)] = dict(points=len(rows), range_bits=[min(bits), max(bits)], in_gap_mean=float(np.mean(gaps)),
                                                in_gap_max=int(max(gaps)), queries_with_a_gap=int(sum(1 for g in gaps if g)))
    for k, v in out.items():
        print(k, json.dumps(v))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
