"""The cases of tests/test_gpu_live_exit.py, shared with tests/golden/make_live_exit_golden.py (which recorded them on
the commit BEFORE the live-topic kernel shed its per-iteration guard work):
a topical model from the generator of tests/test_gpu_live_topics.py (every topic with a vocabulary of its own, so that
documents converge before the iteration cap), 96 documents whose distinct-term counts sit at the
boundaries of the kernel's term slots per lane (65 / 128 / 129 / 192 / 193 / 208 / 256: two, three and four slots, padded
slots of one real term and of none), four stop thresholds crossed with three hand-over counts (option compact_cap).

Per case an E-step on the training fast path (doc_values = 0: the document terms are left to doc_terms_kernel) and one
with per-document values (doc_values = 1: the kernel's own epilogue), each as the SHA-256 of its arrays' bytes.  Plain
module, no GPU."""
import hashlib

import numpy as np

from test_gpu_live_topics import topical_corpus

V, D = 6000, 96
LENGTHS = (65, 66, 100, 127, 128, 129, 130, 160, 191, 192, 193, 200, 207, 208, 209, 256)      # six documents each
TOLS = (1e-2, 1e-3, 1e-4, 1e-6)             # (the last one is the default of the E-step)
CAPS = (4, 20, 56)                          # option compact_cap: single body's smallest tile, single stage, pair stage
MODELS = {"K256": 256, "K128": 128}         # K = 128: no pair stage (a wavefront's tile holds every hand-over count)
MAX_ITER = 50
FIELDS_FAST = ("gamma", "iters", "sstats", "joint", "work")
FIELDS_FULL = ("gamma", "iters", "sstats", "joint", "work", "doc_ll")
TOPICS_PER_DOCUMENT = 2

_cache = {}


def inputs(name):
    """ptr, ids, cts, eta, alpha of a model: eta from the topical generator with as many true topics as topics; each
    document draws exactly its number of distinct terms, without replacement, from the words of two of them (counts 1 .. 4)."""
    if name in _cache:
        return _cache[name]
    K = MODELS[name]
    rng = np.random.default_rng(8100 + K)
    eta = topical_corpus(rng, 4, V, K, 50, true_topics=K)[3]
    beta = eta / eta.sum(axis=1, keepdims=True)
    lengths = rng.permutation(np.repeat(LENGTHS, D // len(LENGTHS)))
    ptr, ids, cts = [0], [], []
    for n in lengths:
        topics = rng.choice(K, size=TOPICS_PER_DOCUMENT, replace=False)
        p = rng.dirichlet(np.full(TOPICS_PER_DOCUMENT, 1.0)) @ beta[topics]
        u = np.sort(rng.choice(V, size=int(n), replace=False, p=p / p.sum()))
        ids.append(u.astype(np.int32))
        cts.append(rng.integers(1, 5, size=int(n)).astype(np.int32))
        ptr.append(ptr[-1] + int(n))
    out = (np.array(ptr, np.int64), np.concatenate(ids), np.concatenate(cts), eta, np.full(K, 1.0 / K))
    for a in out:
        a.setflags(write=False)
    _cache[name] = out
    return out


def reference(name, tol):
    """The C oracle's E-step of a model at a threshold: computed once, shared, never modified."""
    from oracle import c_oracle
    key = (name, tol)
    if key not in _cache:
        ptr, ids, cts, eta, alpha = inputs(name)
        ref = c_oracle.e_step(alpha, eta, ptr, ids, cts, MAX_ITER, tol)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(capi, name, tol, options, fast):
    """One E-step of a model: dict of the arrays, the joint value, the executed work and what the kernels flagged."""
    ptr, ids, cts, eta, alpha = inputs(name)
    ctx = capi.Context(MODELS[name], V)
    for option, value in options:
        ctx.set_option(option, value)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    ctx.work_counters()
    out = ctx.estep_host(corpus, alpha, eta, MAX_ITER, tol, False, want_doc_values=not fast)
    ctx.work_counters()
    if fast:
        out["iters"] = ctx.get_doc_values(corpus, want_ll=False)[2]
    out["joint"] = np.array([out["document_log_likelihood"]])
    out["work"] = np.array(ctx.executed_work())
    out["handed_over"] = out["work"][1]
    out["stop_sums"] = ctx.stop_sum_counters() if hasattr(ctx, "stop_sum_counters") else None
    out["flagged"] = ctx.estep_results(corpus)[2]
    corpus.close()
    ctx.close()
    return out


def digests(out, fast):
    return {field: digest(out[field]) for field in (FIELDS_FAST if fast else FIELDS_FULL)}


def key_of(name, cap, tol, fast, field):
    return "%s/cap%d/tol%g/%s/%s" % (name, cap, tol, "fast" if fast else "full", field)


# ---- the document whose normaliser leaves the fp64 range INSIDE the live-topic kernel (option compact_underflow_doc) ----
# alpha = 1e-3: t of a dead topic, exp(psi(1e-3) - psi(sum gamma)) ~ e^-1000, is an exact zero, so the exactness guard's two
# bounds hold whatever the normalisers are, and the range check is the only thing that can flag a document
UNDERFLOW_MODEL, UNDERFLOW_ALPHA, UNDERFLOW_CAP, UNDERFLOW_N = "K256", 1e-3, 56, 65


def underflow_inputs():
    """The K = 256 model at alpha = 1e-3, and the first of its documents of 65 terms: two term slots per lane, the second
    holding the document's last term - the one the hook scales - on lane 0 beside 63 padded slots that repeat it."""
    ptr, ids, cts, eta, alpha = inputs(UNDERFLOW_MODEL)
    doc = int(np.nonzero(np.diff(ptr) == UNDERFLOW_N)[0][0])
    return (ptr, ids, cts, eta, np.full_like(alpha, UNDERFLOW_ALPHA)), doc


def underflow_reference():
    from oracle import c_oracle
    if "underflow" not in _cache:
        (ptr, ids, cts, eta, alpha), _ = underflow_inputs()
        _cache["underflow"] = c_oracle.e_step(alpha, eta, ptr, ids, cts, MAX_ITER, 1e-6)
    return _cache["underflow"]


def run_underflow(capi, hook, fast):
    """The E-step of underflow_inputs() with the hook on its document (or off): as run(), and per-document `flagged_docs`
    is not reported by the library - the count is (estep_results)."""
    (ptr, ids, cts, eta, alpha), doc = underflow_inputs()
    ctx = capi.Context(MODELS[UNDERFLOW_MODEL], V)
    ctx.set_option("compact_cap", UNDERFLOW_CAP)
    if hook:
        ctx.set_option("compact_underflow_doc", doc)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    ctx.work_counters()
    out = ctx.estep_host(corpus, alpha, eta, MAX_ITER, 1e-6, False, want_doc_values=not fast)
    ctx.work_counters()
    if fast:
        out["iters"] = ctx.get_doc_values(corpus, want_ll=False)[2]
    out["joint"] = np.array([out["document_log_likelihood"]])
    out["work"] = np.array(ctx.executed_work())
    out["handed_over"] = out["work"][1]
    out["flagged"] = ctx.estep_results(corpus)[2]
    corpus.close()
    ctx.close()
    return out


def stops_before_the_cap(iters):
    return int(np.count_nonzero(np.asarray(iters) < MAX_ITER))
