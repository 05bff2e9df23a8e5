"""The sharded collapsed Gibbs engine without a GPU: its numpy restatement (tests/gibbs_sharded_restatement.py) against
the whole-corpus chain (tests/gibbs_restatement.py) token for token, and the --gibbs_sharded flag of the command line."""
import numpy as np
import pytest

import gibbs_restatement as spec
import gibbs_sharded_restatement as sharded

K, SEED, CHECKED_SWEEPS = 10, 31, (1, 2, 5)
_whole = {}


def _documents(ap_train):
    """40 associated-press documents, the shortest with at least 20 tokens, in corpus order (the chains below cost a
    python step per token)."""
    ptr, ids, cts = (np.asarray(ap_train[k]) for k in ("doc_ptr", "term_id", "term_ct"))
    tokens = np.add.reduceat(cts, ptr[:-1])
    tokens[np.diff(ptr) == 0] = 0
    candidates = np.nonzero(tokens >= 20)[0]
    chosen = np.sort(candidates[np.argsort(tokens[candidates], kind="stable")[:40]])
    new_ptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[chosen])]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[d], ptr[d + 1]) for d in chosen])
    return new_ptr, ids[take].astype(np.int32), cts[take].astype(np.int32)


def _priors(V):
    return np.full(K, 0.1), np.full(V, 0.01)


def _whole_states(ap_train, blocks):
    """(z, T, n_k) of the whole-corpus chain after the checked sweeps; computed once per number of blocks."""
    if blocks not in _whole:
        csr, V = _documents(ap_train), len(ap_train["words"])
        chain = spec.GibbsChain(*csr, K, V, seed=SEED)
        chain.init()
        states = {0: (chain.z.copy(), chain.T.copy(), chain.n_k[0].copy())}
        for sweep in range(1, max(CHECKED_SWEEPS) + 1):
            chain.sweep(*_priors(V), blocks, sweep)
            if sweep in CHECKED_SWEEPS:
                states[sweep] = (chain.z.copy(), chain.T.copy(), chain.n_k[0].copy())
        _whole[blocks] = states
    return _whole[blocks]


@pytest.mark.parametrize("blocks", [1, 7, 64])
@pytest.mark.parametrize("cuts", [[0, 17, 40], [0, 9, 26, 40]])
def test_shards_that_exchange_records_are_the_whole_chain(ap_train, cuts, blocks):
    csr, V = _documents(ap_train), len(ap_train["words"])
    want = _whole_states(ap_train, blocks)
    chain = sharded.ShardedChain(*csr, K, V, SEED, cuts)
    chain.init()

    def same(sweep):
        z, T, n_k = want[sweep]
        assert np.array_equal(chain.topics(), z), "sweep %d: %d topics differ" % (sweep, int(np.sum(chain.topics() != z)))
        for s in chain.shards:
            assert np.array_equal(s.T, T) and np.array_equal(s.n_k[0], n_k), sweep
    same(0)
    for sweep in range(1, max(CHECKED_SWEEPS) + 1):
        chain.sweep(*_priors(V), blocks, sweep)
        if sweep in CHECKED_SWEEPS:
            same(sweep)
    assert not np.array_equal(want[0][0], want[5][0])


def test_record_format_and_padding():
    rec = sharded.pack_records([5, 70000, 3], [1, 1023, 4], [2, 0, 4])
    assert rec.dtype == np.uint64
    assert rec.tolist() == [(5 << 32) | (1 << 16) | 2, (70000 << 32) | (1023 << 16), (3 << 32) | (4 << 16) | 4]
    T, n_k = np.zeros((70001, 1024), dtype=np.int64), np.zeros(1024, dtype=np.int64)
    sharded.apply_records(T, n_k, np.concatenate([rec, np.zeros(3, dtype=np.uint64)]))      # (zeros: padding, no move)
    assert T[5, 1] == -1 and T[5, 2] == 1 and T[70000, 1023] == -1 and T[70000, 0] == 1 and np.abs(T).sum() == 4
    assert n_k[1] == -1 and n_k[2] == 1 and n_k[1023] == -1 and n_k[0] == 1 and np.abs(n_k).sum() == 4


class _Launched(Exception):
    pass


def test_command_line_shards_mode_1_only_when_asked(tmp_path, capsys, monkeypatch):
    from pylda_amd import cli
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    launched = []

    def no_exec(program, argv):
        launched.append(list(argv))
        raise _Launched()
    monkeypatch.setattr(cli.os, "execv", no_exec)
    base = ["--input_directory=%s" % tmp_path, "--output_directory=%s" % tmp_path, "--number_of_topics=4", "--training_iterations=2",
            "--inference_mode=1", "--sampler_seed=4", "--gibbs_blocks=16", "--gpus=2"]
    assert cli.train_main(base) == 2 and not launched
    err = capsys.readouterr().err
    assert "one GPU" in err and "--gibbs_sharded=1" in err and "replica" in err and "collectives per sweep" in err
    assert cli.train_main(base + ["--gibbs_sharded=0"]) == 2 and not launched
    with pytest.raises(_Launched):                      # past the mode-1 check: it becomes the launcher of two ranks
        cli.train_main(base + ["--gibbs_sharded=1"])
    assert len(launched) == 1 and "--gibbs_sharded=1" in launched[0] and "--nproc-per-node" in launched[0]
    monkeypatch.setenv("WORLD_SIZE", "2")               # a launcher's ranks without the flag are refused too
    assert cli.train_main(base[:-1]) == 2
    assert "--gibbs_sharded=1" in capsys.readouterr().err
    assert cli._parse(cli.TRAIN_FLAGS, base, "launch_train").gibbs_sharded == 0


def test_monte_carlo_takes_a_process_group_and_never_pickles_it():
    from pylda_amd.monte_carlo import MonteCarlo
    m = MonteCarlo(seed=3, blocks=4)
    assert m._process_group is None
    m._process_group = object()                          # (no collective runs before _initialize)
    state = m.__getstate__()
    assert state["_process_group"] is None and state["_exchange"] is None


def test_new_kernels_use_no_scratch():
    """gibbs_pack_kernel and gibbs_record_apply_kernel from the compiler's own assembly: no scratch, full occupancy."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(root, "pylda_amd", "csrc", "launch_gibbs.hip"))).read().splitlines()
    res = kr.resources(lines, "gibbs")
    names = kr.demangle(list(res))
    found = {}
    for mangled, info in res.items():
        for kernel in ("gibbs_pack_kernel", "gibbs_record_apply_kernel"):
            if kernel in names[mangled]:
                found[kernel] = info
    assert sorted(found) == ["gibbs_pack_kernel", "gibbs_record_apply_kernel"], sorted(names.values())
    for kernel, info in found.items():
        assert info["ScratchSize"] == 0 and info["NumVgprs"] <= 64 and info["Occupancy"] >= 8, (kernel, info)
