#!/usr/bin/env python3
"""Records tests/golden/live_exit_k256.npz on an MI355X: the cases of tests/live_exit_cases.py as the commit BEFORE the
live-topic kernel shed its per-iteration guard work ran them (estep_limits.h live_stop_shortcut and its neighbours) -
or, the same arithmetic, a build of a later tree with the PYLDA_LIVE_... macros at 0.

    python tests/golden/make_live_exit_golden.py [--package-root DIR] [--out FILE] [--commit HASH]

DIR: a checkout or copy whose pylda_amd (built) is recorded instead of this tree's; HASH: the commit DIR holds (kept in
the file as `recorded_from`).  Per model, hand-over count and threshold: the SHA-256 of gamma, the iteration counts, the
statistics, the joint value and the executed work of an E-step on the training fast path and of one with per-document
values (there with the per-document log-likelihood); the documents handed over; and what option compact_guard_fail
flags.  Every case is run twice and must repeat itself bit for bit."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--out", default=os.path.join(HERE, "live_exit_k256.npz"))
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(args.package_root))

from pylda_amd import _capi  # noqa: E402
import live_exit_cases as cases  # noqa: E402

record = {}
for name in cases.MODELS:
    for cap in cases.CAPS:
        for tol in cases.TOLS:
            for fast in (True, False):
                out = cases.run(_capi, name, tol, (("compact_cap", cap),), fast)
                again = cases.run(_capi, name, tol, (("compact_cap", cap),), fast)
                assert out["flagged"] == 0
                for field, d in cases.digests(out, fast).items():
                    assert d == cases.digests(again, fast)[field], (name, cap, tol, fast, field)
                    record[cases.key_of(name, cap, tol, fast, field)] = np.array(d.encode())
                record[cases.key_of(name, cap, tol, fast, "handed_over")] = np.array(out["handed_over"])
            print("%s compact_cap %d tol %g: handed over %d, of all documents %d stop before the cap" %
                  (name, cap, tol, out["handed_over"], cases.stops_before_the_cap(out["iters"])), flush=True)
    for fast in (True, False):
        out = cases.run(_capi, name, 1e-6, (("compact_guard_fail", 1),), fast)
        for field, d in cases.digests(out, fast).items():
            record[cases.key_of(name, 0, 1e-6, fast, "guard_fail/" + field)] = np.array(d.encode())
        record[cases.key_of(name, 0, 1e-6, fast, "guard_fail/flagged")] = np.array(out["flagged"])
        record[cases.key_of(name, 0, 1e-6, fast, "guard_fail/handed_over")] = np.array(out["handed_over"])
        print("%s compact_guard_fail: handed over %d, flagged %d" % (name, out["handed_over"], out["flagged"]), flush=True)
# the document whose normaliser underflows inside the live-topic kernel: needs the test hook compact_underflow_doc, so DIR
# is the parent commit's kernels with the hook's host code (launch_compact.hip, context.hip, host_internal.h) of this tree
for fast in (True, False):
    plain, out = cases.run_underflow(_capi, False, fast), cases.run_underflow(_capi, True, fast)
    assert plain["flagged"] == 0 and plain["handed_over"] == out["handed_over"], (plain["flagged"], plain["handed_over"], out["handed_over"])
    for field, d in cases.digests(out, fast).items():
        record[cases.key_of("underflow", cases.UNDERFLOW_CAP, 1e-6, fast, field)] = np.array(d.encode())
    record[cases.key_of("underflow", cases.UNDERFLOW_CAP, 1e-6, fast, "flagged")] = np.array(out["flagged"])
    record[cases.key_of("underflow", cases.UNDERFLOW_CAP, 1e-6, fast, "handed_over")] = np.array(out["handed_over"])
    print("underflow hook: handed over %d, flagged %d (without the hook %d)" % (out["handed_over"], out["flagged"], plain["flagged"]), flush=True)
np.savez_compressed(args.out, recorded_from=np.array(args.commit.encode()), **record)
print("wrote", args.out, "from", os.path.dirname(_capi.__file__))
