#!/usr/bin/env python3
"""Records tests/golden/quad_handover_pairs.npz on an MI355X: the cases of tests/quad_handover_pairs_cases.py as the
commit BEFORE the hand-over tile went out in slot pairs ran them (estep_limits.h quad_handover_pairs) - or, the same code,
a build of a later tree with -DPYLDA_QUAD_HANDOVER_PAIRS=0.

    python tests/golden/make_quad_handover_pairs_golden.py [--package-root DIR] [--out FILE] [--commit HASH]

DIR: a checkout or copy whose pylda_amd (built) is recorded instead of this tree's; HASH: the commit DIR holds (kept in
the file as `recorded_from`).  Per case (K, compact_cap, path): the SHA-256 of gamma, of the iteration counts and of the
statistics, the joint value and the executed work (tile entries, documents handed over); and per K the hand-over count
at which the last document leaves with every column of its tile in use (`last_cap/K`, cases.cap_met_exactly), with the
same values at that count."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--out", default=os.path.join(HERE, "quad_handover_pairs.npz"))
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(args.package_root))

from pylda_amd import _capi  # noqa: E402
import quad_handover_pairs_cases as cases  # noqa: E402

rec = {}
for K in cases.KS:
    inputs = cases.corpus(K)
    last_cap = cases.cap_met_exactly(cases.live_counts(_capi, K, cases.last_document(inputs)))
    rec["last_cap/%d" % K] = np.array(last_cap)
    print("K %d: the 161-term document meets the hand-over count exactly at %d" % (K, last_cap))
    for cap in cases.CAPS + (last_cap,):
        for path in cases.PATHS:
            out = cases.run(_capi, K, inputs, cap, path)
            assert out["flagged"] == 0
            for field in ("gamma", "iters", "sstats"):
                rec[cases.key(K, cap, path, field)] = np.array(cases.digest(out[field]).encode())
            rec[cases.key(K, cap, path, "joint")] = out["joint"]
            rec[cases.key(K, cap, path, "work")] = out["work"]
            print("K %d compact_cap %d %s: handed over %d, tile entries %d" % (K, cap, path, out["work"][1], out["work"][0]))
np.savez_compressed(args.out, recorded_from=np.array(args.commit.encode()), **rec)
print("wrote", args.out, "from", os.path.dirname(_capi.__file__))
