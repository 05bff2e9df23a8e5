#!/usr/bin/env python3
"""Sub-phase timing of the quad kernel's PROLOGUE and of its HAND-OVER EXIT with s_memtime stamps (development tool).

    python tools/phase_stamps_quad.py [--tag=NAME] [-DNAME=value ...]      # builds an instrumented COPY under .ab/NAME (dbgq)
    (on the GPU)  cd .ab/dbgq && python run_dbg.py [cfg3|cfg4] [nmin nmax]
    (on the GPU)  cd .ab/dbgq && python run_dbg.py handover [cfg3|cfg4] [nmin nmax]

The copy is compiled with -DPYLDA_QUAD_STAMPS=1 (estep_quad.h QUAD_PROLOGUE_*, tools/quad_stamps.h); the working tree's
library is not touched.  run_dbg.py runs the class of documents with nmin .. nmax distinct terms (default 193 .. 208)
of the benchmark's corpus with option quad_packed 0 and 1 (compact = 0, doc_values = 0: every document leaves through
the exit that dumps the stamps) and prints shader ticks per document and sub-phase, for the first and the last
wavefront of a document.  `handover` first trains eta for six outer iterations on the class with the dense kernels
(compact = 0, per-document values: results are right there), so that topics die as they do in the benchmark's window,
then runs one E-step with the hand-over on and prints, over the documents handed over, the ticks of the exit in three
parts (tools/quad_stamps.h): barriers and pos[], the tile stores, the rest."""
import os, shutil, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = next((a[6:] for a in sys.argv[1:] if a.startswith("--tag=")), "dbgq")
flags = [a for a in sys.argv[1:] if not a.startswith("--tag=")]
dst = os.path.join(root, ".ab", tag)
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
handover = bool(args) and args[0] == "handover"
if handover:
    args.pop(0)
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
if handover:
    ctx = _capi.Context(K, V)
    ctx.set_option("compact", 0)
    corpus = ctx.corpus(newptr, ids[idx], cts[idx])
    alpha = np.full(K, 1.0 / K)
    ctx.set_alpha(alpha)
    for outer in range(6):
        ctx.set_eta(eta)
        ctx.estep(corpus)
        eta = 0.01 + ctx.get_sstats()
    live = (ctx.get_gamma(corpus) != alpha).sum(axis=1)
    ctx.set_eta(eta)
    for name, value in (("compact", 1), ("doc_values", 0)):
        ctx.set_option(name, value)
    ctx.estep(corpus)
    g = ctx.get_gamma(corpus)
    print(cfg, "documents", len(sel), "live topics at the end of a dense E-step: mean %.1f, at most %d" % (live.mean(), live.max()),
          "classes", [(c["kernel"], c["geometry"], c["documents"]) for c in corpus.plan()])
    parts = ["entry -> barriers, pos[] done", "-> tile stores landed", "-> the rest"]
    handed = g[:, 5] == -1.0
    print("  handed over %d of %d, at iteration %.2f on average" % (handed.sum(), len(sel), g[handed, 4].mean() if handed.any() else 0))
    for w in (0, W - 1):
        base = 16 * w
        assert np.array_equal(g[:, base + 5] == -1.0, handed)
        print("  wavefront %d" % w)
        for j, nm in enumerate(parts):
            print("     %-34s %9.1f" % (nm, g[handed, base + 6 + j].mean()))
        print("     %-34s %9.1f" % ("exit", g[handed, base + 6:base + 9].sum(axis=1).mean()))
    stores = np.stack([g[handed, 16 * w + 7] for w in range(W)], axis=1)
    print("  tile stores, slowest wavefront of a document: %9.1f" % stores.max(axis=1).mean())
    corpus.close(); ctx.close()
    sys.exit(0)
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
                       "import sys; sys.path.insert(0, %r); from pylda_amd import build; build.build(force=True, verbose=False, extra_flags=['-DPYLDA_QUAD_STAMPS=1'] + %r)" % (dst, flags)])
print("built", dst)
