"""Comparisons against the goldens of the reference's hybrid.py (tests/golden/make_hybrid_golden.py), shared by the CPU
test of the numpy restatement and the GPU test of the kernel."""
import numpy as np

Z = 5.0


def replicated_document(golden):
    """CSR of the moments golden's document (grouped order) replicated `replicas` times."""
    terms, counts, R = golden["terms"], golden["counts"], int(golden["replicas"])
    n = terms.size
    return (np.arange(R + 1, dtype=np.int64) * n, np.tile(terms, R).astype(np.int32), np.tile(counts, R).astype(np.int32))


def moment_failures(golden, mode, gamma, doc_values, stats_mean=None):
    """Where (gamma, per-document likelihood, statistics) differ from the reference's moments by more than 5 sigma.
    gamma (R, K) and doc_values (R,) per replica (document log-likelihood in training mode, words log-likelihood in
    held-out mode); stats_mean (K, terms): the statistics of the document's terms divided by R.  Returns a list of
    strings, empty when everything is within 5 sigma."""
    R, B = int(golden["replicas"]), int(golden["batches"])
    bad = []
    ref_m, ref_v = golden[mode + "_gamma_mean"], golden[mode + "_gamma_var"]
    m, v = gamma.mean(axis=0), gamma.var(axis=0, ddof=1)
    z = np.abs(m - ref_m) / np.sqrt(ref_v / R + v / R)
    if np.any(z > Z):
        bad.append("gamma mean z=%s" % np.round(z, 2))
    ref_ll = golden[mode + "_batch_ll"]
    mine = doc_values.reshape(B, R // B).sum(axis=1)
    zl = abs(mine.mean() - ref_ll.mean()) / np.sqrt(ref_ll.var(ddof=1) / B + mine.var(ddof=1) / B)
    if zl > Z:
        bad.append("batch likelihood %.3f vs %.3f (z=%.2f)" % (mine.mean(), ref_ll.mean(), zl))
    if stats_mean is not None:
        ref_s = golden[mode + "_batch_stats"]
        sigma = np.sqrt(2.0 * ref_s.var(axis=0, ddof=1) / B)
        over = np.abs(stats_mean - ref_s.mean(axis=0)) > Z * sigma + 1e-9
        if np.any(over):
            bad.append("statistics of %d (topic, term) pairs beyond 5 sigma" % int(over.sum()))
    return bad


def trace_band(golden):
    """(lo, hi) per iteration for the joint log-likelihood and for sum(alpha): the reference seeds' range widened by three
    times its spread on each side."""
    out = {}
    for key, values in (("joint_ll", golden["joint_ll"]), ("alpha_sum", golden["alpha"].sum(axis=2))):
        lo, hi = values.min(axis=0), values.max(axis=0)
        out[key] = (lo - 3 * (hi - lo), hi + 3 * (hi - lo))
    return out
