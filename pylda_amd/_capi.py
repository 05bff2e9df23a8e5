"""ctypes binding of libpylda_hip.so (the C ABI in include/pylda_hip.h).

This is the only place Python touches the native library.  There is no CPU
fallback anywhere in pylda_amd: if the shared library is missing, or no HIP
device is visible, the failure is raised here, loudly.
"""
import collections
import ctypes
import os
import threading

import numpy as np

ABI_VERSION = 10         # == PYLDA_ABI_VERSION of include/pylda_hip.h (checked at load time)
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpylda_hip.so")
_lib = None

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int32_p = ctypes.POINTER(ctypes.c_int32)
_c_int64_p = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol include/pylda_hip.h declares
SIGNATURES = {
    "pylda_version": (ctypes.c_char_p, []),
    "pylda_abi_version": (ctypes.c_int, []),
    "pylda_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "pylda_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "pylda_destroy": (None, [_vp]),
    "pylda_last_error": (ctypes.c_char_p, [_vp]),
    "pylda_set_stream": (ctypes.c_int, [_vp, _vp]),
    "pylda_use_own_stream": (ctypes.c_int, [_vp]),
    "pylda_synchronize": (ctypes.c_int, [_vp]),
    "pylda_corpus_create": (ctypes.c_int, [_vp, ctypes.c_int64, _c_int64_p, _c_int32_p, _c_int32_p,
                                           ctypes.POINTER(_vp)]),
    "pylda_corpus_destroy": (None, [_vp]),
    "pylda_corpus_info": (ctypes.c_int, [_vp, _c_int64_p, _c_int64_p, _c_int64_p, _c_int32_p]),
    "pylda_set_eta": (ctypes.c_int, [_vp, _c_double_p]),
    "pylda_get_eta": (ctypes.c_int, [_vp, _c_double_p]),
    "pylda_set_alpha": (ctypes.c_int, [_vp, _c_double_p]),
    "pylda_estep": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_int]),
    "pylda_estep_results": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_int64_p]),
    "pylda_get_sstats": (ctypes.c_int, [_vp, _c_double_p]),
    "pylda_set_sstats": (ctypes.c_int, [_vp, _c_double_p]),
    "pylda_get_gamma": (ctypes.c_int, [_vp, _vp, _c_double_p]),
    "pylda_get_doc_values": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_int32_p]),
    "pylda_estep_host": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_int, _c_double_p, _c_double_p,
                                        _c_double_p, _c_double_p, _c_int32_p, _c_double_p]),
    "pylda_table_stride": (ctypes.c_int, [_vp]),
    "pylda_compute_units": (ctypes.c_int, [_vp]),
    "pylda_sstats_device": (_vp, [_vp]),
    "pylda_eta_device": (_vp, [_vp]),
    "pylda_gamma_device": (_vp, [_vp]),
    "pylda_mark_device_state": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "pylda_comm_unique_id": (ctypes.c_int, [_vp]),
    "pylda_comm_init": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "pylda_comm_destroy": (ctypes.c_int, [_vp]),
    "pylda_allreduce_sstats": (ctypes.c_int, [_vp]),
    "pylda_allreduce_doubles": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int64]),
    "pylda_mstep": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_mstep_enqueue": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                           ctypes.c_double]),
    "pylda_mstep_online": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_double, ctypes.c_double, _c_double_p, _c_double_p]),
    "pylda_mstep_online_enqueue": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_double, ctypes.c_double]),
    "pylda_outer_device": (_vp, [_vp, _c_int64_p]),
    "pylda_allreduce_outer": (ctypes.c_int, [_vp]),
    "pylda_outer_fetch": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_int64_p, _c_double_p, _c_double_p,
                                         _c_double_p]),
    "pylda_host_alloc": (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(_vp)]),
    "pylda_host_free": (ctypes.c_int, [_vp]),
    "pylda_model_checkpoint": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pylda_mark_time": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pylda_elapsed_ms": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "pylda_work_counters": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pylda_executed_work": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pylda_stop_sum_counters": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pylda_clock_counters": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pylda_kernel_time": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_int64_p]),
    "pylda_corpus_layout": (ctypes.c_int64, [_vp, ctypes.c_char_p]),
    "pylda_corpus_plan": (ctypes.c_int, [_vp, ctypes.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_int64_p,
                                         _c_double_p]),
    "pylda_set_option": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    "pylda_parse_corpus": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p,
                                          ctypes.c_int64, ctypes.c_int, _c_int64_p, _c_int64_p, _c_int64_p,
                                          _c_int32_p, _c_int32_p, _c_int64_p]),
    "pylda_test_alpha_update": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                                               ctypes.c_int, ctypes.c_double, _c_double_p]),
    "pylda_test_expdigamma": (ctypes.c_int, [_vp, ctypes.c_int64, _c_double_p, ctypes.c_double, _c_double_p]),
    "pylda_test_special_forms": (ctypes.c_int, [_vp, ctypes.c_int64, _c_double_p, ctypes.c_double, ctypes.c_int, _c_double_p]),
    "pylda_test_tables": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                         _c_double_p, ctypes.POINTER(ctypes.c_int)]),
    "pylda_test_alpha_statistics": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int64, _c_double_p]),
    "pylda_test_statistics": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_int32_p, ctypes.POINTER(ctypes.c_uint16),
                                             _c_double_p, _c_double_p]),
    "pylda_test_special": (ctypes.c_int, [_vp, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_test_gibbs_posterior_terms": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_hybrid_estep": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.c_int64, ctypes.c_int]),
    "pylda_hybrid_scale_sstats": (ctypes.c_int, [_vp, ctypes.c_double]),
    "pylda_test_philox": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32),
                                         ctypes.POINTER(ctypes.c_uint32)]),
    "pylda_gibbs_init": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int64]),
    "pylda_gibbs_sweep": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_int64, ctypes.c_uint64,
                                         ctypes.c_uint64, ctypes.c_int64]),
    "pylda_gibbs_log_posterior": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_gibbs_get_counts": (ctypes.c_int, [_vp, _vp, _c_int32_p, _c_int32_p, _c_int32_p]),
    "pylda_gibbs_set_state": (ctypes.c_int, [_vp, _vp, _c_int32_p, _c_int32_p, _c_int32_p]),
    "pylda_gibbs_round_tokens": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _c_int64_p]),
    "pylda_gibbs_exchange_prepare": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _c_int64_p,
                                                    ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "pylda_gibbs_round_sample": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64]),
    "pylda_gibbs_round_apply": (ctypes.c_int, [_vp, _vp, ctypes.c_int64]),
    "pylda_gibbs_table_device": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _c_int64_p, ctypes.POINTER(_vp)]),
    "pylda_gibbs_log_posterior_parts": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_foldin_set_model": (ctypes.c_int, [_vp, _vp, _c_int32_p, _c_int32_p, _c_double_p, ctypes.c_double]),
    "pylda_foldin": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.c_int64, _c_double_p]),
    "pylda_completion_set_model": (ctypes.c_int, [_vp]),
    "pylda_completion_score": (ctypes.c_int, [_vp, _vp, _vp, _c_double_p, _c_double_p, _c_int64_p]),
    "pylda_left_to_right": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                           ctypes.c_int64, ctypes.c_int64, _c_double_p, _c_int64_p]),
    "pylda_test_left_to_right_state": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), _c_double_p]),
    "pylda_top_words": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, _c_int32_p, _c_double_p]),
    "pylda_codocument_counts": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _c_int32_p, _c_int64_p, _c_int64_p]),
    "pylda_similarity_set_base": (ctypes.c_int, [_vp, ctypes.c_int64, _c_double_p, ctypes.c_int]),
    "pylda_similar_documents": (ctypes.c_int, [_vp, ctypes.c_int64, _c_double_p, ctypes.c_int, ctypes.c_int, _c_int32_p, _c_int32_p,
                                               _c_double_p]),
    "pylda_topic_distances": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "pylda_scvb_init": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int64]),
    "pylda_scvb_step": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_double_p, _c_double_p, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_double_p, _c_double_p]),
    "pylda_scvb_get_state": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_scvb_set_state": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p]),
}
# ... and the collapsed variational Bayes engine's.  A table of its own: tests/test_capi_symbols.py reads the header's names
# as runs of letters and underscores, which "cvb0" is not, and compares them with SIGNATURES; tests/test_cvb0_host.py
# compares these with the header.  load() binds both tables.
CVB0_SIGNATURES = {
    "pylda_cvb0_init": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int64]),
    "pylda_cvb0_sweep": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int64]),
    "pylda_cvb0_log_likelihood": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.c_double, _c_double_p, _c_double_p]),
    "pylda_cvb0_get_state": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_cvb0_set_state": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "pylda_cvb0_foldin": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64,
                                         _c_double_p]),
    "pylda_test_cvb0_postings": (ctypes.c_int, [ctypes.c_int64, _c_int64_p, _c_int32_p, ctypes.c_int64, ctypes.c_int64, _c_int64_p,
                                                _c_int64_p, _c_int64_p, _c_int64_p, _c_int64_p, _c_int32_p, _c_int64_p]),
}


def library_path():
    return _LIB_PATH


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same
    SONAME as the system one).  If this library pulled in the system copy first, a later
    `import torch` would load the bundled copy as a SECOND runtime and fail with "no
    ROCm-capable device".  Loading torch's copy first (when torch is installed; torch itself is
    not imported) makes both resolve to the same runtime, whatever the import order - which is
    also what lets the context run on torch's streams for the RCCL all-reduce.
    PYLDA_HIP_RUNTIME=system skips this (a host process that never imports torch; tested in
    tests/test_gpu_estep.py::test_runs_on_the_system_hip_runtime_without_torch)."""
    if os.environ.get("PYLDA_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        bundled = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(bundled):
            ctypes.CDLL(bundled, mode=ctypes.RTLD_GLOBAL)
    except Exception:           # no torch, or an unexpected layout: the system runtime is used
        pass


def _bind(lib, path=_LIB_PATH, signatures=None):
    """Give every function of `signatures` (None: SIGNATURES) on the library object `lib` its types.  The ABI version moves only when an
    existing entry point changes, so a library built before an addition still passes the version check: a symbol it
    lacks gets the version mismatch's answer - rebuild - not a bare AttributeError."""
    for name, (restype, argtypes) in (SIGNATURES if signatures is None else signatures).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError("pylda_amd: %s does not export %s, which this binding declares: it was built from older "
                               "sources - rebuild it (python -m pylda_amd.build --force)" % (path, name))
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def load():
    """Load libpylda_hip.so; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            "pylda_amd: %s is missing - build it with `python -m pylda_amd.build` "
            "(or __graft_entry__.build()).  pylda_amd has no CPU fallback." % _LIB_PATH)
    _preload_torch_hip_runtime()
    lib = _bind(_bind(ctypes.CDLL(_LIB_PATH)), signatures=CVB0_SIGNATURES)
    if lib.pylda_abi_version() != ABI_VERSION:
        raise RuntimeError("pylda_amd: %s implements ABI %d, this binding was written for ABI %d - rebuild it "
                           "(python -m pylda_amd.build --force)" % (_LIB_PATH, lib.pylda_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(_c_double_p) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(_c_int32_p) if a is not None else None


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
    return a


class _PinnedBlock(object):
    """A page-locked host allocation exposed to numpy (array interface); goes back to the pool when the last
    array viewing it is garbage-collected."""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            _pinned_release(self.ptr, self.nbytes)
        except Exception:
            pass


# Idle page-locked blocks, oldest first: (pointer, nbytes).  The pool is bounded by BYTES, not by count per size - a
# long-running process that asks for many different shapes (inference() on corpora of varying D) must not accumulate
# page-locked memory - and arrays above _PINNED_MAX_ARRAY (the 2 GB gamma of a 1M-document corpus) are never pinned.
# __del__ of a block may run at any garbage-collection point, on any thread, also while pinned_empty() scans the list:
# one re-entrant lock around every access (re-entrant: a collection triggered inside the locked region may release a
# block on the same thread).
_pinned_idle = collections.deque()
_pinned_idle_bytes = 0
_pinned_lock = threading.RLock()
_PINNED_POOL_CAP = 1 << 30          # idle page-locked bytes kept for reuse (least recently released go first)
_PINNED_MAX_ARRAY = 1 << 29         # larger arrays come from ordinary (pageable) memory


def _pinned_release(ptr, nbytes):
    global _pinned_idle_bytes
    evicted = []
    with _pinned_lock:
        _pinned_idle.append((ptr, nbytes))
        _pinned_idle_bytes += nbytes
        while _pinned_idle and _pinned_idle_bytes > _PINNED_POOL_CAP:
            old_ptr, old_bytes = _pinned_idle.popleft()
            _pinned_idle_bytes -= old_bytes
            evicted.append(old_ptr)
    for old_ptr in evicted:                 # (the driver call outside the lock)
        if _lib is not None:
            _lib.pylda_host_free(_vp(old_ptr))


def pinned_pool_bytes():
    """Page-locked bytes currently idle in the pool (for tests and diagnostics)."""
    return _pinned_idle_bytes


def pinned_empty(shape, dtype=np.float64):
    """numpy.empty in page-locked host memory (pylda_host_alloc): the arrays e_step() / m_step() hand back and
    forth move at the PCIe rate.  Recycled through a small pool - page-locking 50 MB costs milliseconds - that is
    capped at _PINNED_POOL_CAP idle bytes; very large arrays and failed allocations fall back to numpy.empty."""
    global _pinned_idle_bytes
    lib = load()
    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    if nbytes == 0 or nbytes > _PINNED_MAX_ARRAY:
        return np.empty(shape, dtype=dtype)
    ptr = None
    with _pinned_lock:
        for i in range(len(_pinned_idle) - 1, -1, -1):      # most recently released block of exactly this size
            if _pinned_idle[i][1] == nbytes:
                ptr = _pinned_idle[i][0]
                del _pinned_idle[i]
                _pinned_idle_bytes -= nbytes
                break
    if ptr is None:
        handle = _vp()
        rc = lib.pylda_host_alloc(nbytes, ctypes.byref(handle))
        if rc != 0:                          # (no page-locked memory left: ordinary memory works everywhere)
            return np.empty(shape, dtype=dtype)
        ptr = handle.value
    return np.asarray(_PinnedBlock(ptr, nbytes)).view(dtype).reshape(shape)


class PyldaError(RuntimeError):
    def __init__(self, status, message):
        RuntimeError.__init__(self, "pylda_hip error %d: %s" % (status, message))
        self.status = status


def _join_documents(lines):
    """One bytes object + the separator byte: a byte that occurs in no document (so a document
    that itself contains line breaks stays ONE document, as in the reference's per-string loop)."""
    for sep in ("\x00", "\x01", "\x02", "\x03"):      # never white space, (almost) never in text
        text = sep.join(lines)
        if text.count(sep) == max(len(lines) - 1, 0):
            return text.encode("utf-8", "surrogatepass"), ord(sep)
    # every candidate occurs somewhere: 0xFF is not a byte of any UTF-8 sequence
    return b"\xff".join(l.encode("utf-8", "surrogatepass") for l in lines), 0xFF


def parse_corpus(lines, vocabulary, lowercase=False):
    """Native parse_data (variational_bayes.py:98-130): documents (iterable of str) and the
    vocabulary in id order -> CSR (doc_ptr int64, term_id int32, term_ct int32), #dropped.

    A vocabulary entry that is empty or contains white space can never equal a token of
    str.split(); it keeps its id (a placeholder no token can match takes its line)."""
    lib = load()
    lines = list(lines)
    text, sep = _join_documents(lines)
    vocab = b"\n".join(w.encode("utf-8", "surrogatepass") if len(w.split()) == 1 and w == w.strip()
                       else b"\xfe%d" % i for i, w in enumerate(vocabulary))
    n_docs, nnz = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.pylda_parse_corpus(text, len(text), sep, vocab, len(vocab), 1 if lowercase else 0,
                                ctypes.byref(n_docs), ctypes.byref(nnz), None, None, None, None)
    if rc != 0:
        raise PyldaError(rc, "pylda_parse_corpus (sizing pass)")
    doc_ptr = np.zeros(n_docs.value + 1, dtype=np.int64)
    term_id = np.zeros(max(nnz.value, 1), dtype=np.int32)
    term_ct = np.zeros(max(nnz.value, 1), dtype=np.int32)
    rc = lib.pylda_parse_corpus(text, len(text), sep, vocab, len(vocab), 1 if lowercase else 0,
                                ctypes.byref(n_docs), ctypes.byref(nnz),
                                doc_ptr.ctypes.data_as(_c_int64_p), term_id.ctypes.data_as(_c_int32_p),
                                term_ct.ctypes.data_as(_c_int32_p), None)
    if rc != 0:
        raise PyldaError(rc, "pylda_parse_corpus")
    return doc_ptr, term_id[:nnz.value], term_ct[:nnz.value], len(lines) - n_docs.value


def comm_unique_id():
    """128 opaque bytes naming a new RCCL communicator (call on rank 0, hand to every rank)."""
    lib = load()
    buf = ctypes.create_string_buffer(128)
    rc = lib.pylda_comm_unique_id(ctypes.cast(buf, _vp))
    if rc != 0:
        raise PyldaError(rc, (lib.pylda_last_error(None) or b"").decode())
    return buf.raw


def device_count():
    n = ctypes.c_int(0)
    load().pylda_device_count(ctypes.byref(n))
    return n.value


class Context(object):
    """A model-sized device context: K topics over V word types on one GPU."""

    def __init__(self, number_of_topics, number_of_types, device=0):
        lib = load()
        handle = _vp()
        rc = lib.pylda_create(int(device), int(number_of_topics), int(number_of_types),
                              ctypes.byref(handle))
        if rc != 0:
            raise PyldaError(rc, (lib.pylda_last_error(None) or b"").decode())
        self._lib = lib
        self._h = handle
        self.K = int(number_of_topics)
        self.V = int(number_of_types)
        self.device = int(device)

    def _check(self, rc):
        if rc != 0:
            raise PyldaError(rc, (self._lib.pylda_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pylda_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- model state ----
    def set_eta(self, eta):
        self._check(self._lib.pylda_set_eta(self._h, _dp(_f64(eta, (self.K, self.V), "eta"))))

    def get_eta(self):
        out = pinned_empty((self.K, self.V))
        self._check(self._lib.pylda_get_eta(self._h, _dp(out)))
        return out

    def set_alpha(self, alpha):
        self._check(self._lib.pylda_set_alpha(self._h, _dp(_f64(alpha, (self.K,), "alpha"))))

    def set_stream(self, hip_stream):
        """Run on the HIP stream with this handle; 0 / None is the device's default (null) stream."""
        self._check(self._lib.pylda_set_stream(self._h, _vp(hip_stream) if hip_stream else None))

    def use_own_stream(self):
        self._check(self._lib.pylda_use_own_stream(self._h))

    def synchronize(self):
        self._check(self._lib.pylda_synchronize(self._h))

    def set_option(self, name, value):
        self._check(self._lib.pylda_set_option(self._h, name.encode(), int(value)))

    # ---- corpus ----
    def corpus(self, doc_ptr, term_id, term_ct):
        return Corpus(self, doc_ptr, term_id, term_ct)

    # ---- hot path ----
    def estep(self, corpus, max_iter=50, tol=1e-6, heldout=False):
        self._check(self._lib.pylda_estep(self._h, corpus._h, int(max_iter), float(tol),
                                          1 if heldout else 0))

    def estep_results(self, corpus):
        ll, wll, nlog = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._lib.pylda_estep_results(self._h, corpus._h, ctypes.byref(ll),
                                                  ctypes.byref(wll), ctypes.byref(nlog)))
        return ll.value, wll.value, nlog.value

    def get_sstats(self):
        out = pinned_empty((self.K, self.V))
        self._check(self._lib.pylda_get_sstats(self._h, _dp(out)))
        return out

    def set_sstats(self, sstats):
        self._check(self._lib.pylda_set_sstats(self._h, _dp(_f64(sstats, (self.K, self.V), "sstats"))))

    def get_gamma(self, corpus):
        out = pinned_empty((corpus.D, self.K))
        self._check(self._lib.pylda_get_gamma(self._h, corpus._h, _dp(out)))
        return out

    def get_doc_values(self, corpus, want_ll=True):
        """(doc_ll, doc_words_ll, iters) of the last E-step; want_ll=False skips the per-document
        likelihoods (unavailable after an E-step on the training fast path, option doc_values=0)."""
        ll = np.empty(corpus.D, dtype=np.float64) if want_ll else None
        wll = np.empty(corpus.D, dtype=np.float64) if want_ll else None
        iters = np.empty(corpus.D, dtype=np.int32)
        self._check(self._lib.pylda_get_doc_values(self._h, corpus._h, _dp(ll), _dp(wll), _ip(iters)))
        return ll, wll, iters

    def estep_host(self, corpus, alpha, eta, max_iter=50, tol=1e-6, heldout=False,
                   want_doc_values=True):
        """One-shot form: returns a dict of host arrays."""
        alpha = _f64(alpha, (self.K,), "alpha")
        eta = _f64(eta, (self.K, self.V), "eta")
        gamma = np.empty((corpus.D, self.K), dtype=np.float64)
        sstats = None if heldout else np.empty((self.K, self.V), dtype=np.float64)
        ll = np.empty(corpus.D) if want_doc_values else None
        wll = np.empty(corpus.D) if want_doc_values else None
        iters = np.empty(corpus.D, dtype=np.int32) if want_doc_values else None
        scal = np.zeros(2)
        self.set_option("doc_values", 1 if want_doc_values else 0)
        self._check(self._lib.pylda_estep_host(
            self._h, corpus._h, _dp(alpha), _dp(eta), int(max_iter), float(tol),
            1 if heldout else 0, _dp(gamma), _dp(sstats), _dp(ll), _dp(wll), _ip(iters), _dp(scal)))
        return {"document_log_likelihood": scal[0], "words_log_likelihood": scal[1],
                "gamma": gamma, "sstats": sstats, "doc_ll": ll, "doc_words_ll": wll, "iters": iters}

    def hybrid_estep(self, corpus, number_of_samples=10, burn_in_samples=5, seed=0, stream=0, first_document=0,
                     heldout=False):
        """The hybrid (Gibbs-within-VB) E-step, enqueued: gamma, per-document values and scalars as after estep();
        in training mode the sufficient statistics are raw sample counts until hybrid_scale_sstats()."""
        self._check(self._lib.pylda_hybrid_estep(self._h, corpus._h, int(number_of_samples), int(burn_in_samples),
                                                 int(seed) & (2 ** 64 - 1), int(stream), int(first_document),
                                                 1 if heldout else 0))

    def hybrid_scale_sstats(self, divisor):
        self._check(self._lib.pylda_hybrid_scale_sstats(self._h, float(divisor)))

    def test_philox(self, counter_key):
        """Philox4x32-10 on the device: (n, 6) uint32 records (counter 0..3, key 0..1) -> (n, 4) uint32 blocks."""
        rec = np.ascontiguousarray(counter_key, dtype=np.uint32).reshape(-1, 6)
        out = np.empty((rec.shape[0], 4), dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self._lib.pylda_test_philox(self._h, rec.shape[0], rec.ctypes.data_as(u32p), out.ctypes.data_as(u32p)))
        return out

    # ---- collapsed Gibbs engine (the state lives in the corpus) ----
    def gibbs_init(self, corpus, seed=0, first_document=0):
        """Every token's topic uniformly at random, then n_dk, the word-topic counts and n_k."""
        self._check(self._lib.pylda_gibbs_init(self._h, corpus._h, int(seed) & (2 ** 64 - 1), int(first_document)))

    def gibbs_sweep(self, corpus, alpha, beta, blocks, seed=0, stream=1, first_document=0):
        """One sweep of `blocks` block-synchronous rounds, enqueued; beta_sum is numpy.sum(beta)."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        self._check(self._lib.pylda_gibbs_sweep(self._h, corpus._h, _dp(alpha), _dp(beta), float(np.sum(beta)), int(blocks),
                                                int(seed) & (2 ** 64 - 1), int(stream), int(first_document)))

    def gibbs_log_posterior(self, corpus, alpha, beta):
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        out = ctypes.c_double(0)
        self._check(self._lib.pylda_gibbs_log_posterior(self._h, corpus._h, _dp(alpha), _dp(beta), ctypes.byref(out)))
        return out.value

    def gibbs_get_counts(self, corpus, want_n_kv=True, want_topics=True):
        """(n_kv (K, V) int32 or None, n_k (K,) int32, the tokens' topics int32 or None)."""
        n_kv = np.empty((self.K, self.V), dtype=np.int32) if want_n_kv else None
        n_k = np.empty(self.K, dtype=np.int32)
        topics = np.empty(corpus.tokens, dtype=np.int32) if want_topics else None
        self._check(self._lib.pylda_gibbs_get_counts(self._h, corpus._h, _ip(n_kv), _ip(n_k), _ip(topics)))
        return n_kv, n_k, topics

    def gibbs_set_state(self, corpus, n_kv=None, n_k=None, topics=None):
        """Restore the word-topic counts, n_k and / or the tokens' topics (n_dk follows from the topics)."""
        def i32(a, shape, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.int32)
            if a.shape != tuple(shape):
                raise ValueError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
            return a
        n_kv, n_k = i32(n_kv, (self.K, self.V), "n_kv"), i32(n_k, (self.K,), "n_k")
        topics = i32(topics, (corpus.tokens,), "topics")
        self._check(self._lib.pylda_gibbs_set_state(self._h, corpus._h, _ip(n_kv), _ip(n_k), _ip(topics)))

    # ---- ... sharded over several ranks: a round is round_sample, an all-gather of the records, round_apply ----
    def gibbs_round_tokens(self, corpus, blocks, first_document=0):
        """int64 (blocks,): the tokens of this corpus in each round's block."""
        tokens = np.zeros(int(blocks), dtype=np.int64)
        self._check(self._lib.pylda_gibbs_round_tokens(self._h, corpus._h, int(blocks), int(first_document),
                                                       tokens.ctypes.data_as(_c_int64_p)))
        return tokens

    def gibbs_exchange_prepare(self, corpus, blocks, first_document, world, rank, capacity):
        """The record buffers for `capacity[g]` records per rank in round g; returns the device addresses (send, recv).
        A second call frees what the first returned."""
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        if capacity.shape != (int(blocks),):
            raise ValueError("capacity has shape %s, expected %s" % (capacity.shape, (int(blocks),)))
        send, recv = _vp(), _vp()
        self._check(self._lib.pylda_gibbs_exchange_prepare(self._h, corpus._h, int(blocks), int(first_document), int(world), int(rank),
                                                           capacity.ctypes.data_as(_c_int64_p), ctypes.byref(send), ctypes.byref(recv)))
        return int(send.value or 0), int(recv.value or 0)

    def gibbs_round_sample(self, corpus, alpha, beta, blocks, round, seed=0, stream=1, first_document=0):
        """The sampler on the corpus' documents of the round's block, then their move records into the send buffer."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        self._check(self._lib.pylda_gibbs_round_sample(self._h, corpus._h, _dp(alpha), _dp(beta), float(np.sum(beta)), int(blocks),
                                                       int(round), int(seed) & (2 ** 64 - 1), int(stream), int(first_document)))

    def gibbs_round_apply(self, corpus, round):
        """Every rank's records of the round, from the receive buffer, into the corpus' table and n_k."""
        self._check(self._lib.pylda_gibbs_round_apply(self._h, corpus._h, int(round)))

    def gibbs_table_device(self, corpus):
        """(device address of the word-major int32 table, its elements, device address of n_k)."""
        table, n_k, elements = _vp(), _vp(), ctypes.c_int64(0)
        self._check(self._lib.pylda_gibbs_table_device(self._h, corpus._h, ctypes.byref(table), ctypes.byref(elements), ctypes.byref(n_k)))
        return int(table.value or 0), int(elements.value), int(n_k.value or 0)

    def gibbs_log_posterior_parts(self, corpus, alpha, beta):
        """(the documents' part, the words' and n_k's part) of gibbs_log_posterior."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        out = np.zeros(2, dtype=np.float64)
        self._check(self._lib.pylda_gibbs_log_posterior_parts(self._h, corpus._h, _dp(alpha), _dp(beta), _dp(out)))
        return float(out[0]), float(out[1])

    # ---- held-out fold-in against a frozen Gibbs model (the model lives in the context) ----
    def foldin_set_model(self, beta, trained=None, n_kv=None, n_k=None):
        """The predictive table from a trained corpus' Gibbs state on the device, or from host counts n_kv (K, V), n_k (K);
        beta_sum is numpy.sum(beta)."""
        beta = _f64(beta, (self.V,), "beta")
        if trained is None:
            n_kv, n_k = np.ascontiguousarray(n_kv, dtype=np.int32), np.ascontiguousarray(n_k, dtype=np.int32)
            if n_kv.shape != (self.K, self.V) or n_k.shape != (self.K,):
                raise ValueError("n_kv, n_k have shapes %s, %s, expected %s, %s" % (n_kv.shape, n_k.shape, (self.K, self.V), (self.K,)))
        self._check(self._lib.pylda_foldin_set_model(self._h, trained._h if trained is not None else None,
                                                     _ip(n_kv) if trained is None else None, _ip(n_k) if trained is None else None,
                                                     _dp(beta), float(np.sum(beta))))

    def foldin(self, corpus, alpha, number_of_samples=50, burn_in_samples=25, seed=0, stream=0, first_document=0):
        """Folds the corpus' documents into the model; returns words_log_likelihood (gamma: get_gamma, the per-document
        likelihoods: get_doc_values()[1])."""
        alpha = _f64(alpha, (self.K,), "alpha")
        out = ctypes.c_double(0)
        self._check(self._lib.pylda_foldin(self._h, corpus._h, _dp(alpha), int(number_of_samples), int(burn_in_samples),
                                           int(seed) & (2 ** 64 - 1), int(stream), int(first_document), ctypes.byref(out)))
        return out.value

    # ---- collapsed variational Bayes, CVB0 (the state lives in the corpus) ----
    def cvb0_init(self, corpus, seed=0, first_document=0):
        """Every copy's topic uniformly at random as gibbs_init draws it; a slot's row is its copies' histogram / their number."""
        self._check(self._lib.pylda_cvb0_init(self._h, corpus._h, int(seed) & (2 ** 64 - 1), int(first_document)))

    def cvb0_sweep(self, corpus, alpha, beta, blocks, first_document=0):
        """One sweep of block-synchronous rounds, enqueued; beta_sum is numpy.sum(beta)."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        self._check(self._lib.pylda_cvb0_sweep(self._h, corpus._h, _dp(alpha), _dp(beta), float(np.sum(beta)), int(blocks),
                                               int(first_document)))

    def cvb0_log_likelihood(self, corpus, alpha, beta):
        """(the training plug-in log-likelihood, the last sweep's sum of c |new row - old row|)."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        ll, change = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.pylda_cvb0_log_likelihood(self._h, corpus._h, _dp(alpha), _dp(beta), float(np.sum(beta)),
                                                        ctypes.byref(ll), ctypes.byref(change)))
        return ll.value, change.value

    def cvb0_get_state(self, corpus, want_n_kv=True, want_g=True):
        """(n_kv (K, V) or None, n_k (K,), n_dk (D, K), g (nnz, K) or None), float64."""
        n_kv = np.empty((self.K, self.V)) if want_n_kv else None
        n_k, n_dk = np.empty(self.K), np.empty((corpus.D, self.K))
        g = np.empty((corpus.nnz, self.K)) if want_g else None
        self._check(self._lib.pylda_cvb0_get_state(self._h, corpus._h, _dp(n_kv), _dp(n_k), _dp(n_dk), _dp(g)))
        return n_kv, n_k, n_dk, g

    def cvb0_set_state(self, corpus, n_kv=None, n_k=None, n_dk=None, g=None):
        """Restore the table, n_k, n_dk and / or the slots' rows, each as given."""
        def f64(a, shape, name):
            return None if a is None else _f64(a, shape, name)
        n_kv, n_k = f64(n_kv, (self.K, self.V), "n_kv"), f64(n_k, (self.K,), "n_k")
        n_dk, g = f64(n_dk, (corpus.D, self.K), "n_dk"), f64(g, (corpus.nnz, self.K), "g")
        self._check(self._lib.pylda_cvb0_set_state(self._h, corpus._h, _dp(n_kv), _dp(n_k), _dp(n_dk), _dp(g)))

    def cvb0_foldin(self, corpus, alpha, sweeps=50, seed=0, stream=0, first_document=0):
        """Folds the corpus' documents into the context's predictive table; returns words_log_likelihood (gamma: get_gamma,
        the per-document likelihoods: get_doc_values()[1])."""
        alpha = _f64(alpha, (self.K,), "alpha")
        out = ctypes.c_double(0)
        self._check(self._lib.pylda_cvb0_foldin(self._h, corpus._h, _dp(alpha), int(sweeps), int(seed) & (2 ** 64 - 1), int(stream),
                                                int(first_document), ctypes.byref(out)))
        return out.value

    # ---- stochastic collapsed variational Bayes, SCVB0 (the state lives in the corpus; no per-slot rows) ----
    def scvb_init(self, corpus, seed=0, first_document=0):
        """cvb0_init's start without the slots' rows: the table, n_k and N_dk are the histograms of the drawn topics."""
        self._check(self._lib.pylda_scvb_init(self._h, corpus._h, int(seed) & (2 ** 64 - 1), int(first_document)))

    def scvb_step(self, corpus, block, batches, alpha, beta, keep, gain, rho_theta, first_document=0):
        """One minibatch step on block `block` of `batches`, enqueued: len(rho_theta) = burn_in + 1 passes per document, then
        table = keep * table + gain * (the block's expected counts).  beta_sum is numpy.sum(beta); 1 - rho_theta is formed
        here, in double."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        rho_theta = _f64(rho_theta, name="rho_theta").reshape(-1)
        one_minus = _f64([1.0 - float(rho) for rho in rho_theta])
        self._check(self._lib.pylda_scvb_step(self._h, corpus._h, int(block), int(batches), int(first_document), _dp(alpha), _dp(beta),
                                              float(np.sum(beta)), float(keep), float(gain), len(rho_theta), _dp(rho_theta),
                                              _dp(one_minus)))

    def scvb_get_state(self, corpus, want_n_kv=True):
        """(n_kv (K, V) or None, n_k (K,), n_dk (D, K), doc_change (D,): every document's sum_k |N_dk after - before| of its
        last visit), float64."""
        n_kv = np.empty((self.K, self.V)) if want_n_kv else None
        n_k, n_dk, doc_change = np.empty(self.K), np.empty((corpus.D, self.K)), np.empty(corpus.D)
        self._check(self._lib.pylda_scvb_get_state(self._h, corpus._h, _dp(n_kv), _dp(n_k), _dp(n_dk), _dp(doc_change)))
        return n_kv, n_k, n_dk, doc_change

    def scvb_set_state(self, corpus, n_kv=None, n_k=None, n_dk=None):
        """Restore the table, n_k and / or n_dk, each as given."""
        def f64(a, shape, name):
            return None if a is None else _f64(a, shape, name)
        n_kv, n_k, n_dk = f64(n_kv, (self.K, self.V), "n_kv"), f64(n_k, (self.K,), "n_k"), f64(n_dk, (corpus.D, self.K), "n_dk")
        self._check(self._lib.pylda_scvb_set_state(self._h, corpus._h, _dp(n_kv), _dp(n_k), _dp(n_dk)))

    # ---- document-completion held-out likelihood (the table lives in the context, beside / in place of fold-in's) ----
    def completion_set_model(self):
        """The predictive table P[w][k] = eta[k][w] / sum_v eta[k][v] from the device eta, enqueued."""
        self._check(self._lib.pylda_completion_set_model(self._h))

    def completion_score(self, held, observed=None, gamma=None):
        """Scores the held corpus under the gamma in `observed`'s device buffer, or under the host array `gamma` (D, K);
        returns (held_log_likelihood, held_tokens).  The per-document values: get_doc_values(held)[1]."""
        if gamma is not None:
            gamma = _f64(gamma, (held.D, self.K), "gamma")
        ll, tokens = ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._lib.pylda_completion_score(self._h, observed._h if observed is not None else None, held._h, _dp(gamma),
                                                     ctypes.byref(ll), ctypes.byref(tokens)))
        return ll.value, tokens.value

    # ---- left-to-right held-out likelihood (reads the predictive table either set-model call built) ----
    def left_to_right(self, corpus, alpha, particles=20, resample=True, seed=0, stream=0, first_document=0, step_budget=0):
        """log p(w | Phi, alpha) of the corpus' documents by the left-to-right estimator; returns (log_likelihood, tokens).
        The per-document estimates: get_doc_values(corpus)[1].  step_budget 0: the library's default."""
        alpha = _f64(alpha, (self.K,), "alpha")
        ll, tokens = ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._lib.pylda_left_to_right(self._h, corpus._h, _dp(alpha), int(particles), int(resample),
                                                  int(seed) & (2 ** 64 - 1), int(stream), int(first_document), int(step_budget),
                                                  ctypes.byref(ll), ctypes.byref(tokens)))
        return ll.value, tokens.value

    def test_left_to_right_state(self, corpus, particles):
        """(z uint16, p float64), both flat (tokens * particles,), of the last left_to_right call on `corpus`: document d's
        topics at [first token * R, (first token + N_d) * R) as (R, N_d), its p as (N_d, R)."""
        cells = int(corpus.tokens) * int(particles)
        z, p = np.empty(cells, dtype=np.uint16), np.empty(cells, dtype=np.float64)
        self._check(self._lib.pylda_test_left_to_right_state(self._h, corpus._h, int(particles),
                                                             z.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), _dp(p)))
        return z, p

    # ---- topic coherence: the top words of every topic, the co-document counts of their pairs ----
    def top_words(self, M, table=None):
        """(top_ids (K, M) int32, top_values (K, M) float64): the first M entries of every row of `table` (K, V) - None:
        the device eta - larger value first, among equal values the smaller word id first."""
        if table is not None:
            table = _f64(table, (self.K, self.V), "table")
        M = int(M)
        ids = np.empty((self.K, max(M, 0)), dtype=np.int32)
        values = np.empty((self.K, max(M, 0)), dtype=np.float64)
        self._check(self._lib.pylda_top_words(self._h, _dp(table), M, _ip(ids), _dp(values)))
        return ids, values

    def codocument_counts(self, corpus, ids):
        """(doc_freq (K, M) int64, co_doc_freq (K, M, M) int64) of the word ids (K, M) over the documents of `corpus`: the
        documents that contain a word, and those that contain both words of a pair."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != self.K:
            raise ValueError("ids has shape %s, expected (%d, M)" % (ids.shape, self.K))
        M = ids.shape[1]
        doc_freq = np.empty((self.K, M), dtype=np.int64)
        co = np.empty((self.K, M, M), dtype=np.int64)
        self._check(self._lib.pylda_codocument_counts(self._h, corpus._h, M, _ip(ids), doc_freq.ctypes.data_as(_c_int64_p),
                                                      co.ctypes.data_as(_c_int64_p)))
        return doc_freq, co

    # ---- nearest documents by topic mixture: a base of rows on the device, the first N of it for every query ----
    def similarity_set_base(self, rows, transform):
        """Upload `rows` (D, K) as the base of similar_documents.  transform 0: as given, 1: theta = row / its sum, 2: sqrt(theta)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.K:
            raise ValueError("rows has shape %s, expected (D, %d)" % (rows.shape, self.K))
        self._check(self._lib.pylda_similarity_set_base(self._h, rows.shape[0], _dp(rows), int(transform)))

    def similar_documents(self, rows, N, transform, self_ids=None):
        """(ids (Q, N) int32, scores (Q, N) float64): for every query row the first N documents of the base by the score
        sum_k a_k b_k - larger first, equal scores by the smaller index - leaving out document self_ids[q] (-1: none).
        Fewer than N candidates: trailing ids -1, scores -inf."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.K:
            raise ValueError("rows has shape %s, expected (Q, %d)" % (rows.shape, self.K))
        Q, N = rows.shape[0], int(N)
        if self_ids is not None:
            self_ids = np.ascontiguousarray(self_ids, dtype=np.int32)
            if self_ids.shape != (Q,):
                raise ValueError("self_ids has shape %s, expected (%d,)" % (self_ids.shape, Q))
        ids = np.empty((Q, max(N, 0)), dtype=np.int32)
        scores = np.empty((Q, max(N, 0)), dtype=np.float64)
        self._check(self._lib.pylda_similar_documents(self._h, Q, _dp(rows), int(transform), N, _ip(self_ids), _ip(ids), _dp(scores)))
        return ids, scores

    # ---- topic distances between two models: the rows of two (K', V) tables as distributions over the words ----
    def topic_distances(self, a=None, b=None, metric=1):
        """(Ka, Kb) float64: metric 0 the Bhattacharyya coefficients, 1 the Jensen-Shannon divergences (nats) between the
        rows of `a` (Ka, V) - None: the device eta - and of `b` (Kb, V) - None: `a` against itself."""
        tables = []
        for name, table in (("a", a), ("b", b)):
            if table is not None:
                table = np.ascontiguousarray(table, dtype=np.float64)
                if table.ndim != 2 or table.shape[1] != self.V:
                    raise ValueError("%s has shape %s, expected (K', %d)" % (name, table.shape, self.V))
            tables.append(table)
        a, b = tables
        Ka = a.shape[0] if a is not None else self.K
        Kb = b.shape[0] if b is not None else Ka
        out = np.empty((Ka, Kb), dtype=np.float64)
        self._check(self._lib.pylda_topic_distances(self._h, _dp(a), Ka, _dp(b), Kb, int(metric), _dp(out)))
        return out

    def mstep(self, corpus, beta, want_alpha_ss=True):
        beta = _f64(beta, (self.V,), "beta")
        tll = ctypes.c_double(0)
        ass = np.empty(self.K, dtype=np.float64) if want_alpha_ss else None
        self._check(self._lib.pylda_mstep(self._h, corpus._h if corpus is not None else None,
                                          _dp(beta), ctypes.byref(tll), _dp(ass)))
        return tll.value, ass

    def mstep_enqueue(self, corpus, beta, hyper_parameter_iteration=0, hyper_parameter_decay_factor=0.9,
                      hyper_parameter_maximum_decay=10, hyper_parameter_converge_threshold=1e-6):
        """The device half of m_step, nothing waited for (see outer_fetch); hyper_parameter_iteration > 0 also
        schedules the alpha update (optimize_hyperparameters) on the device."""
        beta = _f64(beta, (self.V,), "beta")
        self._check(self._lib.pylda_mstep_enqueue(self._h, corpus._h, _dp(beta), int(hyper_parameter_iteration),
                                                  float(hyper_parameter_decay_factor), int(hyper_parameter_maximum_decay),
                                                  float(hyper_parameter_converge_threshold)))

    def mstep_online(self, corpus, beta, rho, scale, want_alpha_ss=True):
        """The M-step of an online step, waited for: eta <- (1 - rho) eta + rho (scale sstats + beta) in place; returns
        (topic log-likelihood of the eta before the blend, alpha statistics of the corpus' gamma or None)."""
        beta = _f64(beta, (self.V,), "beta") if beta is not None else None
        tll = ctypes.c_double(0)
        ass = np.empty(self.K, dtype=np.float64) if want_alpha_ss else None
        self._check(self._lib.pylda_mstep_online(self._h, corpus._h if corpus is not None else None, _dp(beta),
                                                 float(rho), float(scale), ctypes.byref(tll), _dp(ass)))
        return tll.value, ass

    def mstep_online_enqueue(self, corpus, beta, rho, scale):
        """The same, nothing waited for and no alpha update scheduled: outer_fetch returns the minibatch's values."""
        beta = _f64(beta, (self.V,), "beta") if beta is not None else None
        self._check(self._lib.pylda_mstep_online_enqueue(self._h, corpus._h if corpus is not None else None, _dp(beta),
                                                         float(rho), float(scale)))

    def outer_device(self):
        """(device pointer, elements, leading elements that are rank-local sums) of the packed outer-iteration values."""
        n = ctypes.c_int64(0)
        ptr = self._lib.pylda_outer_device(self._h, ctypes.byref(n))
        return int(ptr or 0), 3 * self.K + 4, int(n.value)

    def allreduce_outer(self):
        self._check(self._lib.pylda_allreduce_outer(self._h))

    def outer_fetch(self):
        """(document_log_likelihood, number_of_documents, logspace_documents, topic_log_likelihood, alpha_ss,
        alpha): the one host wait of an outer iteration; alpha is what the device holds now (updated there when
        mstep_enqueue asked for it)."""
        ll, nd, tll, nlog = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        ass, alpha = np.empty(self.K, dtype=np.float64), np.empty(self.K, dtype=np.float64)
        self._check(self._lib.pylda_outer_fetch(self._h, ctypes.byref(ll), ctypes.byref(nd), ctypes.byref(nlog),
                                                ctypes.byref(tll), _dp(ass), _dp(alpha)))
        return ll.value, int(round(nd.value)), nlog.value, tll.value, ass, alpha

    def model_checkpoint(self, restore=False):
        self._check(self._lib.pylda_model_checkpoint(self._h, 1 if restore else 0))

    def mark_time(self, slot):
        self._check(self._lib.pylda_mark_time(self._h, int(slot)))

    def elapsed_ms(self, slot_from, slot_to):
        ms = ctypes.c_double(0)
        self._check(self._lib.pylda_elapsed_ms(self._h, int(slot_from), int(slot_to), ctypes.byref(ms)))
        return ms.value

    def work_counters(self):
        """(sum_d I_d, sum_d I_d N_d) of the profiled E-steps since the last call."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.pylda_work_counters(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def executed_work(self):
        """(tile entries the kernels ran through the FMA pipes, documents handed to the live-topic kernel) of the E-steps
        the LAST work_counters() call read (no device access)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.pylda_executed_work(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def stop_sum_counters(self):
        """(iterations of the live-topic kernel that skipped the stop sum, iterations that formed it) of the E-steps the
        LAST work_counters() call read (no device access)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.pylda_stop_sum_counters(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def shader_clock_mhz(self):
        """Sustained shader clock under the load of the E-steps the last work_counters() call read, or None (no span was
        sampled): resident kernels time themselves in shader cycles and in ticks of the constant-rate counter."""
        a, b, hz = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.pylda_clock_counters(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(hz)))
        return a.value / b.value * hz.value / 1e6 if b.value > 0 else None

    # ---- device-resident interop ----
    def sstats_elements(self):
        """Number of doubles behind sstats_device_ptr(): V * table stride."""
        return self.V * int(self._lib.pylda_table_stride(self._h))

    def compute_units(self):
        """Compute units of the context's device (one workgroup of the statistics pass' persistent sweep each)."""
        return int(self._lib.pylda_compute_units(self._h))

    def sstats_device_ptr(self):
        return int(self._lib.pylda_sstats_device(self._h) or 0)

    def eta_device_ptr(self):
        return int(self._lib.pylda_eta_device(self._h) or 0)

    def mark_device_state(self, have_eta=-1, have_sstats=-1):
        self._check(self._lib.pylda_mark_device_state(self._h, int(have_eta), int(have_sstats)))

    # ---- multi-GPU exchange through the C ABI (RCCL bound at run time; no torch involved) ----
    def comm_init(self, unique_id, rank, world_size):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.pylda_comm_init(self._h, ctypes.cast(buf, _vp), int(rank), int(world_size)))

    def comm_destroy(self):
        self._check(self._lib.pylda_comm_destroy(self._h))

    def allreduce_sstats(self):
        self._check(self._lib.pylda_allreduce_sstats(self._h))

    def allreduce_doubles(self, values):
        values = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._lib.pylda_allreduce_doubles(self._h, _dp(values), values.size))
        return values

    # ---- profiling ----
    def set_profiling(self, enabled):
        self._check(self._lib.pylda_set_profiling(self._h, 1 if enabled else 0))

    def kernel_time(self):
        """(document-kernel ms, statistics-pass ms, E-steps) accumulated since the last call."""
        ms, ss, calls = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._lib.pylda_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(ss), ctypes.byref(calls)))
        return ms.value, ss.value, calls.value

    def test_alpha_update(self, alpha, alpha_ss, number_of_documents, iterations=100, decay_factor=0.9, maximum_decay=10,
                          threshold=1e-6):
        alpha, alpha_ss = _f64(alpha, (self.K,), "alpha"), _f64(alpha_ss, (self.K,), "alpha_ss")
        out = np.empty(self.K, dtype=np.float64)
        self._check(self._lib.pylda_test_alpha_update(self._h, _dp(alpha), _dp(alpha_ss), float(number_of_documents),
                                                      int(iterations), float(decay_factor), int(maximum_decay),
                                                      float(threshold), _dp(out)))
        return out

    def test_alpha_statistics(self, gamma):
        """The M-step's alpha statistics of the rows of `gamma` (D, K) with the context's alpha and the option
        alpha_ss_moved as it stands (pylda_hip.h: pylda_test_alpha_statistics) -> (K,)."""
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        if gamma.ndim != 2 or gamma.shape[1] != self.K:
            raise ValueError("gamma has shape %s, expected (D, %d)" % (gamma.shape, self.K))
        out = np.empty(self.K, dtype=np.float64)
        self._check(self._lib.pylda_test_alpha_statistics(self._h, _dp(gamma), gamma.shape[0], _dp(out)))
        return out

    def test_expdigamma(self, x, c):
        x = _f64(x)
        out = np.empty_like(x)
        self._check(self._lib.pylda_test_expdigamma(self._h, x.size, _dp(x), float(c), _dp(out)))
        return out

    def test_special_forms(self, x, form, c=0.0):
        """One call form of the device special functions at every x (pylda_hip.h lists the forms)."""
        x = _f64(x)
        out = np.empty_like(x)
        self._check(self._lib.pylda_test_special_forms(self._h, x.size, _dp(x), float(c), int(form), _dp(out)))
        return out

    def test_special(self, x):
        x = _f64(x)
        dg, lg = np.empty_like(x), np.empty_like(x)
        self._check(self._lib.pylda_test_special(self._h, x.size, _dp(x), _dp(dg), _dp(lg)))
        return dg, lg

    def test_tables(self, alpha_sgn=False, tables=True, only=None):
        """The tables an E-step prepares from the context's eta (pylda_hip.h: pylda_test_tables), as the device holds them:
        the V x ldk arrays whole, padding columns included; "path": 1 the one-kernel path, 2 the two passes.  alpha_sgn: the
        context's alpha as the live-topic hand-over reads it, too; tables = False: nothing but those two is read back;
        only: the names of the tables to read back (None: all six)."""
        ldk = int(self._lib.pylda_table_stride(self._h))
        out = {}
        if tables:
            out = {"psi_rowsum": (self.K,), "elog": (self.V, ldk), "expElog": (self.V, ldk),
                   "expElog_elog": (self.V, ldk), "shift": (self.V,), "topic_lse": (self.K,)}
            out = {name: np.empty(shape) for name, shape in out.items() if only is None or name in only}
        if alpha_sgn:
            out["alpha_sgn"] = np.empty(self.K)
        path = ctypes.c_int(0)
        self._check(self._lib.pylda_test_tables(self._h, *[_dp(out.get(name)) for name in (
            "psi_rowsum", "elog", "expElog", "expElog_elog", "shift", "topic_lse", "alpha_sgn")], ctypes.byref(path)))
        out["path"] = path.value
        return out

    def test_statistics(self, corpus, t, r, live_n=None, live_topic=None, live_t=None):
        """The statistics pass of `corpus` on given inputs (pylda_hip.h: pylda_test_statistics): t (D, table stride), r (nnz)
        in the order of the corpus' term_id, optionally the documents' lists of live topics - live_n (D), -1: no list,
        live_topic (D, 60) uint16 and live_t (D, 60).  Returns the sum of the entropy partials; the statistics: get_sstats()."""
        ldk = int(self._lib.pylda_table_stride(self._h))
        t, r = _f64(t, (corpus.D, ldk), "t"), _f64(r, (corpus.nnz,), "r")
        topic_p = None
        if live_n is not None:
            live_n = np.ascontiguousarray(live_n, dtype=np.int32)
            live_topic = np.ascontiguousarray(live_topic, dtype=np.uint16)
            live_t = _f64(live_t, (corpus.D, 60), "live_t")
            if live_n.shape != (corpus.D,) or live_topic.shape != (corpus.D, 60):
                raise ValueError("live_n, live_topic have shapes %s, %s, expected %s, %s"
                                 % (live_n.shape, live_topic.shape, (corpus.D,), (corpus.D, 60)))
            topic_p = live_topic.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
        entropy = ctypes.c_double(0)
        self._check(self._lib.pylda_test_statistics(self._h, corpus._h, _dp(t), _dp(r), _ip(live_n), topic_p, _dp(live_t),
                                                    ctypes.byref(entropy)))
        return entropy.value

    def test_gibbs_posterior_terms(self, corpus, alpha, beta):
        """The terms of gibbs_log_posterior on the corpus' state (pylda_hip.h: pylda_test_gibbs_posterior_terms): the
        documents' terms (D), the words' terms (V) and the three device sums - the whole, the documents' half, the words'
        and n_k's half - before the host's scalar terms are added."""
        alpha, beta = _f64(alpha, (self.K,), "alpha"), _f64(beta, (self.V,), "beta")
        docs, words, sums = np.zeros(corpus.D), np.zeros(self.V), np.zeros(3)
        self._check(self._lib.pylda_test_gibbs_posterior_terms(self._h, corpus._h, _dp(alpha), _dp(beta), _dp(docs), _dp(words),
                                                               _dp(sums)))
        return docs, words, sums


class Corpus(object):
    """A parsed corpus resident on the device (CSR of distinct term ids/counts)."""

    def __init__(self, ctx, doc_ptr, term_id, term_ct):
        doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
        term_id = np.ascontiguousarray(term_id, dtype=np.int32)
        term_ct = np.ascontiguousarray(term_ct, dtype=np.int32)
        if doc_ptr.ndim != 1 or doc_ptr.size < 1:
            raise ValueError("doc_ptr must hold D+1 offsets")
        if term_id.shape != term_ct.shape or term_id.ndim != 1 or term_id.size != doc_ptr[-1]:
            raise ValueError("term_id/term_ct must be 1-D of length doc_ptr[-1]")
        handle = _vp()
        rc = ctx._lib.pylda_corpus_create(
            ctx._h, doc_ptr.size - 1, doc_ptr.ctypes.data_as(_c_int64_p),
            term_id.ctypes.data_as(_c_int32_p), term_ct.ctypes.data_as(_c_int32_p),
            ctypes.byref(handle))
        ctx._check(rc)
        self._ctx = ctx
        self._h = handle
        self.D = int(doc_ptr.size - 1)
        self.nnz = int(term_id.size)
        tokens = ctypes.c_int64(0)
        ctx._lib.pylda_corpus_info(handle, None, None, ctypes.byref(tokens), None)      # (summed while validating)
        self.tokens = int(tokens.value)

    def gamma_device_ptr(self):
        return int(self._ctx._lib.pylda_gamma_device(self._h) or 0)

    VARIANT_NAMES = {0: "generic64", 1: "generic256", 2: "generic512", 3: "generic_global", 4: "slab",
                     6: "quilt", 9: "qgroup", 10: "quad", 11: "qfuse", 12: "generic_huge", 13: "qfusek"}

    def plan(self):
        """Launch classes of this corpus: list of dicts (kernel, geometry, documents, terms, kernel_ms)."""
        lib = self._ctx._lib
        n = lib.pylda_corpus_plan(self._h, 0, None, None, None, None, None)
        if n < 0:
            self._ctx._check(n)
        variant, geometry = np.zeros(n, np.int32), np.zeros(n, np.int32)
        documents, terms, ms = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        rc = lib.pylda_corpus_plan(self._h, n, _ip(variant), _ip(geometry), documents.ctypes.data_as(_c_int64_p),
                                   terms.ctypes.data_as(_c_int64_p), _dp(ms))
        if rc < 0:
            self._ctx._check(rc)
        return [{"kernel": self.VARIANT_NAMES.get(int(variant[i]), str(int(variant[i]))), "geometry": int(geometry[i]),
                 "documents": int(documents[i]), "terms": int(terms[i]), "kernel_ms": float(ms[i])}
                for i in range(n)]

    def layout(self, name):
        """Layout facts: "gather_blocks", "gather_segments", "quad_slot_bytes", ... (include/pylda_hip.h)."""
        v = self._ctx._lib.pylda_corpus_layout(self._h, name.encode())
        if v < 0:
            self._ctx._check(int(v))
        return int(v)

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._lib.pylda_corpus_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cvb0_block_postings(doc_ptr, term_id, blocks, first_document=0):
    """The postings cvb0_sweep builds for (blocks, first_document), on the host (pylda_hip.h: pylda_test_cvb0_postings): a
    dict of rounds (n, 6), post_slot, slot_place, seg_begin, run_word, run_seg, widest_postings, widest_segments."""
    lib = load()
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term_id = np.ascontiguousarray(term_id, dtype=np.int32)
    D, nnz = len(doc_ptr) - 1, int(doc_ptr[-1])
    i64 = lambda a: a.ctypes.data_as(_c_int64_p)
    counts = np.zeros(5, dtype=np.int64)
    args = (D, i64(doc_ptr), _ip(term_id), int(blocks), int(first_document))
    if lib.pylda_test_cvb0_postings(*args, i64(counts), None, None, None, None, None, None) != 0:
        raise ValueError("cvb0_block_postings: blocks=%s, first_document=%s" % (blocks, first_document))
    rounds = np.zeros((int(counts[0]), 6), dtype=np.int64)
    post_slot, slot_place = np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.int64)
    seg_begin, run_seg = np.zeros(int(counts[1]) + 1, dtype=np.int64), np.zeros(int(counts[2]) + 1, dtype=np.int64)
    run_word = np.zeros(int(counts[2]), dtype=np.int32)
    lib.pylda_test_cvb0_postings(*args, i64(counts), i64(rounds), i64(post_slot), i64(slot_place), i64(seg_begin), _ip(run_word),
                                 i64(run_seg))
    return {"rounds": rounds, "post_slot": post_slot, "slot_place": slot_place, "seg_begin": seg_begin, "run_word": run_word,
            "run_seg": run_seg, "widest_postings": int(counts[3]), "widest_segments": int(counts[4])}
