#!/usr/bin/env python3
"""Sub-phase timing of the quad kernel's PROLOGUE with s_memtime stamps (development tool).

    python tools/phase_stamps_quad.py [-DNAME=value ...]      # builds an instrumented COPY under .ab/dbgq
    (on the GPU)  cd .ab/dbgq && python run_dbg.py [cfg3|cfg4] [nmin nmax]

The copy is compiled with -DPYLDA_QUAD_STAMPS=1 (estep_quad.h QUAD_PROLOGUE_*, tools/quad_stamps.h); the working tree's
library is not touched.  run_dbg.py runs the class of documents with nmin .. nmax distinct terms (default 193 .. 208)
of the benchmark's corpus with option quad_packed 0 and 1 (compact = 0, doc_values = 0: every document leaves through
the exit that dumps the stamps) and prints shader ticks per document and sub-phase, for the first and the last
wavefront of a document."""
import os, shutil, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dst = os.path.join(root, ".ab", "dbgq")
shutil.rmtree(dst, ignore_errors=True)
os.makedirs(dst)
for d in ("pylda_amd", "include"):
    shutil.copytree(os.path.join(root, d), os.path.join(dst, d), ignore=shutil.ignore_patterns("lib", "__pycache__"))
shutil.copy(os.path.join(root, "tools", "quad_stamps.h"), os.path.join(dst, "pylda_amd", "csrc", "quad_stamps.h"))
open(os.path.join(dst, "run_dbg.py"), "w").write('''
import os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pylda_amd import _capi
from pylda_amd.corpus import synthetic_lda_shard
args = sys.argv[1:]
cfg = args.pop(0) if args and args[0] in ("cfg3", "cfg4") else "cfg4"
nmin, nmax = (int(args.pop(0)), int(args.pop(0))) if len(args) >= 2 and args[0].isdigit() else (193, 208)
D, V, K, seed = (100000, 50000, 128, 1234) if cfg == "cfg3" else (100000, 100000, 256, 5678)
ptr, ids, cts = synthetic_lda_shard(D if cfg == "cfg3" else 1000000, V, 0, D, 128, 200, seed, chunk=25000, device="cuda", workers=8)
n = np.diff(ptr)
sel = np.nonzero((n >= nmin) & (n <= nmax))[0]
newptr = np.concatenate([[0], np.cumsum(n[sel])]).astype(np.int64)
idx = np.concatenate([np.arange(ptr[d], ptr[d + 1]) for d in sel])
np.random.seed(0)
eta = np.random.gamma(100., 0.01, (K, V))
W = 4 if K <= 128 else 8
names = ["entry -> term ids landed", "-> last row landed", "-> first barrier passed", "-> first t stored, last barrier"]
for packed in (0, 1):
    ctx = _capi.Context(K, V)
    for name, value in (("quad_packed", packed), ("compact", 0), ("doc_values", 0)):
        ctx.set_option(name, value)
    corpus = ctx.corpus(newptr, ids[idx], cts[idx])
    ctx.set_alpha(np.full(K, 1.0 / K)); ctx.set_eta(eta)
    ctx.estep(corpus); ctx.estep(corpus)
    g = ctx.get_gamma(corpus)
    print(cfg, "documents", len(sel), "quad_packed", packed, "slot bytes", corpus.layout("quad_slot_bytes"),
          "classes", [(c["kernel"], c["geometry"], c["documents"]) for c in corpus.plan()])
    for w in (0, W - 1):
        base = 16 * w
        print("  wavefront %d (mean iterations %.2f)" % (w, g[:, base + 4].mean()))
        for j, nm in enumerate(names):
            print("     %-34s %9.1f" % (nm, g[:, base + j].mean()))
        print("     %-34s %9.1f" % ("prologue", g[:, base:base + 4].sum(axis=1).mean()))
    corpus.close(); ctx.close()
''')
subprocess.check_call([sys.executable, "-c",
                       "import sys; sys.path.insert(0, %r); from pylda_amd import build; build.build(force=True, verbose=False, extra_flags=['-DPYLDA_QUAD_STAMPS=1'] + %r)" % (dst, sys.argv[1:])])
print("built", dst)
