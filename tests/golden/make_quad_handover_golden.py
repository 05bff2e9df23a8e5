#!/usr/bin/env python3
"""Records tests/golden/quad_handover_k256.npz on an MI355X: the hand-over timing sweep of tests/quad_handover_cases.py
as the commit BEFORE the early hand-over of the quad kernel ran it (estep_limits.h quad_early_handoff) - or, the same
code, a build of a later tree with -DPYLDA_QUAD_EARLY_HANDOFF=0.

    python tests/golden/make_quad_handover_golden.py [--package-root DIR] [--out FILE] [--commit HASH]

DIR: a checkout or copy whose pylda_amd (built) is recorded instead of this tree's; HASH: the commit DIR holds (kept in
the file as `recorded_from`).  The file also holds, for tests/test_gpu_quad_prologue.py, the SHA-256 of gamma, the
per-document log-likelihood, the iteration counts and the statistics of an E-step on the boundary-length corpora of
tests/test_gpu_quad_slots.py at K = 129 / 256 in its four modes, as that commit computed them (before the prologue
requested its loads at once: estep_limits.h quad_prologue_at_once)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--out", default=os.path.join(HERE, "quad_handover_k256.npz"))
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(args.package_root))

from pylda_amd import _capi  # noqa: E402
import quad_handover_cases as cases  # noqa: E402
import test_gpu_quad_slots as slots  # noqa: E402

inputs = slots.boundary_corpus(cases.K)
shape = (len(cases.CAPS), len(cases.TOLS), len(cases.MAX_ITERS))
iters = np.zeros(shape + (slots.D,), np.int32)
entries, handed = np.zeros(shape), np.zeros(shape)
digest = np.zeros(shape, dtype="S64")
for a, cap in enumerate(cases.CAPS):
    for b, tol in enumerate(cases.TOLS):
        for c, out in enumerate(cases.sweep(_capi, inputs, slots.V, (("compact_cap", cap),), tol)):
            assert out["flagged"] == 0
            iters[a, b, c], entries[a, b, c], handed[a, b, c] = out["iters"], out["tile_entries"], out["handed_over"]
            digest[a, b, c] = cases.gamma_digest(out["gamma"]).encode()
        print("compact_cap %d tol %g: handed over" % (cap, tol), handed[a, b].astype(int).tolist())
boundary = {}
for K in cases.BOUNDARY_KS:
    for mode, kw in slots.MODES.items():
        out = slots.run(_capi, K, slots.boundary_corpus(K), 1, **kw)
        assert out["flagged"] == 0 and out["quad_slot_bytes"] > 0
        for name, d in cases.boundary_digests(out, bool(kw.get("heldout"))).items():
            boundary["boundary/%d/%s/%s" % (K, mode, name)] = np.array(d.encode())
np.savez_compressed(args.out, iters=iters, tile_entries=entries, handed_over=handed, gamma_sha256=digest,
                    recorded_from=np.array(args.commit.encode()), **boundary)
print("wrote", args.out, "from", os.path.dirname(_capi.__file__))
