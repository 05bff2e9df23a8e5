"""The collapsed Gibbs engine sharded over several ranks on the GPU.

Part 1, one process and no collective: the shards are corpora of ONE context; what the all-gather would do - every rank's
send segment into every rank's receive buffer - is done with device copies, so pylda_gibbs_round_sample /
pylda_gibbs_round_apply run exactly as under the collective and nothing can wait for a peer.  Part 2: real ranks
(MonteCarlo(process_group=...), launch_train --gibbs_sharded=1), each spawned test under a time limit of its own."""
import os
import pickle
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import gibbs_golden_checks as checks
import gibbs_sharded_restatement as spec
from conftest import rel_err
from test_gpu_gibbs import _ap_text, _case, _synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, OOM, STATE = -1, -3, -4


# ---------------------------------------------------------------------------------------------- part 1: one process
class Shards(object):
    """The shards of a corpus in one context, and the exchange between them by device copies."""

    def __init__(self, ctx, csr, cuts, seed, blocks, extra_capacity=0):
        import torch
        from pylda_amd import distributed
        self.ctx, self.cuts, self.seed = ctx, cuts, seed
        self.world = len(cuts) - 1
        self.rounds = max(1, min(blocks, cuts[-1]))
        self.device = torch.device("cuda", ctx.device)
        self.corpora = [ctx.corpus(*spec.shard_csr(*csr, lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
        for corpus, lo in zip(self.corpora, cuts[:-1]):
            ctx.gibbs_init(corpus, seed, lo)
        # every replica holds the sum of the shards' tables (what allreduce_gibbs_table does over the ranks)
        views = []
        for corpus in self.corpora:
            table, elements, n_k = ctx.gibbs_table_device(corpus)
            assert elements == ctx.sstats_elements()             # (V x the table stride)
            views.append((distributed.device_tensor(table, (elements,), self.device, typestr="<i4"),
                          distributed.device_tensor(n_k, (ctx.K,), self.device, typestr="<i4")))
        with torch.cuda.stream(ctx._torch_stream):
            for part in (0, 1):
                total = sum(v[part] for v in views)
                for v in views:
                    v[part].copy_(total)
        self.tokens = [ctx.gibbs_round_tokens(c, self.rounds, lo) for c, lo in zip(self.corpora, cuts[:-1])]
        self.capacity = np.max(self.tokens, axis=0) + extra_capacity
        self.buffers = []
        widest = int(self.capacity.max())
        for rank, (corpus, lo) in enumerate(zip(self.corpora, cuts[:-1])):
            send, recv = ctx.gibbs_exchange_prepare(corpus, self.rounds, lo, self.world, rank, self.capacity)
            self.buffers.append((distributed.device_tensor(send, (max(widest, 1),), self.device, typestr="<i8"),
                                 distributed.device_tensor(recv, (max(widest, 1) * self.world,), self.device, typestr="<i8")))

    def round(self, alpha, beta, g, stream):
        """Every shard samples against its replica; then every shard receives and applies all segments."""
        import torch
        cap = int(self.capacity[g])
        for corpus, lo in zip(self.corpora, self.cuts[:-1]):
            self.ctx.gibbs_round_sample(corpus, alpha, beta, self.rounds, g, self.seed, stream, lo)
        with torch.cuda.stream(self.ctx._torch_stream):
            for _, recv in self.buffers:
                for rank, (send, _) in enumerate(self.buffers):
                    recv[rank * cap:(rank + 1) * cap].copy_(send[:cap])
        for corpus in self.corpora:
            self.ctx.gibbs_round_apply(corpus, g)

    def sweep(self, alpha, beta, stream):
        for g in range(self.rounds):
            self.round(alpha, beta, g, stream)

    def sent(self, g):
        """What the ranks would receive in round g (uint64), read back from the send buffers."""
        cap = int(self.capacity[g])
        self.ctx.synchronize()
        return np.concatenate([send[:cap].cpu().numpy().view(np.uint64) for send, _ in self.buffers])

    def assert_equal_to(self, whole, what):
        ctx = self.ctx
        n_kv, n_k, topics = ctx.gibbs_get_counts(whole)
        n_dk = np.array(ctx.get_gamma(whole))
        mine = [ctx.gibbs_get_counts(c) for c in self.corpora]
        got = np.concatenate([m[2] for m in mine])
        assert np.array_equal(got, topics), "%s: %d of %d topics differ" % (what, int(np.sum(got != topics)), topics.size)
        for rank, (corpus, m) in enumerate(zip(self.corpora, mine)):
            assert np.array_equal(m[0], n_kv) and np.array_equal(m[1], n_k), "%s: replica %d" % (what, rank)
            rows = np.array(ctx.get_gamma(corpus)).reshape(-1, ctx.K)
            assert np.array_equal(rows, n_dk[self.cuts[rank]:self.cuts[rank + 1]]), "%s: n_dk of shard %d" % (what, rank)
        return topics

    def close(self):
        for c in self.corpora:
            c.close()


def _sharded_case(name, ap_train):
    """(K, V, csr, alpha, beta, blocks, cuts)"""
    if name.startswith("ap400_b"):                               # two unequal halves: a zero tail in every round
        K, V = 10, len(ap_train["words"])
        return K, V, checks.first_documents(ap_train, 400), np.full(K, 0.1), np.full(V, 0.01), int(name.split("_b")[1]), [0, 170, 400]
    if name == "empty_shard":                                    # a rank without documents; 16 rounds, shards of 12 and 18:
        K, V = 10, len(ap_train["words"])                        # rounds whose block is empty on one rank only
        return K, V, checks.first_documents(ap_train, 30), np.full(K, 0.1), np.full(V, 0.01), 16, [0, 12, 12, 30]
    if name in ("k128", "k700"):                                 # vector alpha, vector beta
        K, V, csr, alpha, beta, blocks = _case(name, ap_train)
        return K, V, csr, alpha, beta, blocks, [0, 100, 300] if name == "k128" else [0, 50, 80]
    # a 3000-term document (more than 64 terms per wavefront) next to a term repeated 300 times (many records per term)
    K, V = 32, 4000
    ptr, ids, cts = _synthetic(20, V, 3, 30, 9)
    lp, li, lc = _synthetic(1, V, 3000, 3000, 5)
    ptr = np.concatenate([ptr, ptr[-1] + lp[1:], [ptr[-1] + lp[-1] + 1]])
    ids, cts = np.concatenate([ids, li, [17]]).astype(np.int32), np.concatenate([cts, lc, [300]]).astype(np.int32)
    rng = np.random.default_rng(3)
    return K, V, (ptr, ids, cts), rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V), 3, [0, 21, 22]


@pytest.mark.parametrize("name", ["ap400_b1", "ap400_b16", "ap400_b400", "k128", "k700", "empty_shard", "long_and_repeated"])
def test_shards_equal_the_whole_corpus_on_every_token(name, ap_train):
    from pylda_amd import _capi, distributed
    K, V, csr, alpha, beta, blocks, cuts = _sharded_case(name, ap_train)
    seed = 4321 + len(name)
    ctx = _capi.Context(K, V)
    try:
        distributed.bind_to_torch_stream(ctx)
        whole = ctx.corpus(*csr)
        ctx.gibbs_init(whole, seed)
        shards = Shards(ctx, csr, cuts, seed, blocks, extra_capacity=3 if name == "k128" else 0)
        assert np.any(shards.capacity % 256 != 0) and np.any(shards.capacity * shards.world % 256 != 0)
        assert all(np.any(t < shards.capacity) for t in shards.tokens[1:]) or np.any(shards.tokens[0] < shards.capacity)
        if name == "empty_shard":
            assert any(np.any((t == 0) & (shards.capacity > 0)) for t in shards.tokens)
        start = shards.assert_equal_to(whole, "initial assignment")
        for sweep in range(1, 6):
            ctx.gibbs_sweep(whole, alpha, beta, blocks, seed, sweep)
            shards.sweep(alpha, beta, sweep)
            if sweep in (1, 2, 5):
                topics = shards.assert_equal_to(whole, "sweep %d" % sweep)
        assert not np.array_equal(start, topics)
        # the two parts of the log posterior: the documents' summed over the shards, the replica's once
        want = ctx.gibbs_log_posterior(whole, alpha, beta)
        parts = [ctx.gibbs_log_posterior_parts(c, alpha, beta) for c in shards.corpora]
        assert len(set(p[1] for p in parts)) == 1
        assert rel_err(sum(p[0] for p in parts) + parts[0][1], want) < 1e-12
        assert rel_err(sum(ctx.gibbs_log_posterior_parts(whole, alpha, beta)), want) < 1e-13
        assert ctx.gibbs_log_posterior(whole, alpha, beta) == want
        shards.close()
        whole.close()
    finally:
        ctx.close()


def test_send_buffer_holds_the_restatements_records_word_for_word(ap_train):
    """Three shards of 60 documents, 4 rounds: what every rank would receive in each round of the first sweep equals the
    numpy pack_records output - the record format, the order inside a segment and the zeroed tails."""
    from pylda_amd import _capi, distributed
    K, V, seed, blocks, cuts = 10, len(ap_train["words"]), 99, 4, [0, 13, 40, 60]
    csr = checks.first_documents(ap_train, 60)
    alpha, beta = np.full(K, 0.1), np.full(V, 0.01)
    chain = spec.ShardedChain(*csr, K, V, seed, cuts)
    chain.init()
    ctx = _capi.Context(K, V)
    try:
        distributed.bind_to_torch_stream(ctx)
        shards = Shards(ctx, csr, cuts, seed, blocks)
        moved = 0
        for g in range(blocks):
            want = chain.round(alpha, beta, float(np.sum(beta)), blocks, g, 1)
            shards.round(alpha, beta, g, 1)
            got = shards.sent(g)
            assert got.shape == want.shape and np.array_equal(got, want), "round %d: %d records differ" % (g, int(np.sum(got != want)))
            moved += int(np.sum(((want >> np.uint64(16)) & np.uint64(0xffff)) != (want & np.uint64(0xffff))))
        assert moved > 100
        for s, corpus in zip(chain.shards, shards.corpora):
            n_kv, n_k, topics = ctx.gibbs_get_counts(corpus)
            assert np.array_equal(topics, s.z) and np.array_equal(n_kv, s.T.T) and np.array_equal(n_k, s.n_k[0])
        shards.close()
    finally:
        ctx.close()


def test_call_order_and_argument_errors_are_codes_not_faults(ap_train):
    from pylda_amd import _capi
    K, V, seed = 10, len(ap_train["words"]), 5
    csr = checks.first_documents(ap_train, 20)
    alpha, beta = np.full(K, 0.1), np.full(V, 0.01)
    ctx = _capi.Context(K, V)

    def status(call, *args, **kwargs):
        with pytest.raises(_capi.PyldaError) as e:
            call(*args, **kwargs)
        return e.value.status
    try:
        corpus = ctx.corpus(*csr)
        assert status(ctx.gibbs_table_device, corpus) == STATE                     # no Gibbs state yet
        assert status(ctx.gibbs_log_posterior_parts, corpus, alpha, beta) == STATE
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, 0, seed, 1, 0) == STATE
        assert status(ctx.gibbs_round_apply, corpus, 0) == STATE
        ctx.gibbs_init(corpus, seed)
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, 0, seed, 1, 0) == STATE      # no exchange_prepare yet
        assert status(ctx.gibbs_round_apply, corpus, 0) == STATE
        tokens = ctx.gibbs_round_tokens(corpus, 4, 0)
        assert tokens.sum() == corpus.tokens and np.all(tokens > 0)
        assert status(ctx.gibbs_round_tokens, corpus, 0, 0) == INVALID
        assert status(ctx.gibbs_round_tokens, corpus, 4, -1) == INVALID
        for world, rank in ((0, 0), (2, -1), (2, 2)):
            assert status(ctx.gibbs_exchange_prepare, corpus, 4, 0, world, rank, tokens) == INVALID
        short = tokens.copy()
        short[2] -= 1
        assert status(ctx.gibbs_exchange_prepare, corpus, 4, 0, 1, 0, short) == INVALID        # below the corpus' own count
        assert status(ctx.gibbs_exchange_prepare, corpus, 0, 0, 1, 0, np.zeros(0, np.int64)) == INVALID
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, 0, seed, 1, 0) == STATE  # (none of them left a plan)
        huge = tokens.copy()
        huge[0] = 1 << 36                                                                      # 512 GiB of records to send
        assert status(ctx.gibbs_exchange_prepare, corpus, 4, 0, 2, 0, huge) == OOM
        ctx.gibbs_exchange_prepare(corpus, 4, 0, 1, 0, tokens + 7)
        send, recv = ctx.gibbs_exchange_prepare(corpus, 4, 0, 1, 0, tokens)                    # replaces the first
        assert send and recv and send != recv
        assert status(ctx.gibbs_exchange_prepare, corpus, 4, 0, 2, 0, huge) == OOM             # a refused call ...
        assert status(ctx.gibbs_exchange_prepare, corpus, 4, 0, 1, 0, short) == INVALID
        assert status(ctx.gibbs_round_tokens, corpus, (1 << 24) + 1, 0) == INVALID             # (two host entries per round)
        for bad in (-1, 4, 1 << 40):
            assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, bad, seed, 1, 0) == STATE
            assert status(ctx.gibbs_round_apply, corpus, bad) == STATE
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 5, 0, seed, 1, 0) == STATE  # another number of blocks
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, 0, seed, 1, 3) == STATE  # another offset
        assert status(ctx.gibbs_round_sample, corpus, alpha, beta, 4, 0, seed, 1 << 32, 0) == INVALID
        assert status(ctx.gibbs_round_sample, corpus, alpha, np.zeros(V), 4, 0, seed, 1, 0) == INVALID      # beta_sum = 0
        before = ctx.gibbs_get_counts(corpus)
        ctx.gibbs_round_sample(corpus, alpha, beta, 4, 0, seed, 1, 0)        # ... left the plan in place; (the table waits for round_apply)
        after = ctx.gibbs_get_counts(corpus)
        assert np.array_equal(before[0], after[0]) and not np.array_equal(before[2], after[2])
        corpus.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- part 2: real ranks
SPAWN_LIMIT = 240            # seconds a spawned test may take before its ranks are killed (a run takes ~20)
TRAIN = dict(documents=300, topics=10, blocks=16, iterations=12, interval=5, seed=100)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawn(worker, args, nprocs):
    """mp.spawn under a time limit: ranks whose collectives do not match wait for each other for ever."""
    import torch.multiprocessing as mp
    context = mp.spawn(worker, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + SPAWN_LIMIT
    try:
        while not context.join(timeout=1.0):
            assert time.monotonic() < deadline, "the ranks did not finish within %d s" % SPAWN_LIMIT
    finally:
        for process in context.processes:
            if process.is_alive():
                process.kill()


def _shard_lines(documents, world, rank):
    bounds = [0, 170, len(documents)] if world == 2 else [round(len(documents) * r / world) for r in range(world + 1)]
    return documents[bounds[rank]:bounds[rank + 1]]


def _train(ap_train, group=None, world=1, rank=0, device=0, numpy_seed=0, seed_offset=0):
    from pylda_amd.monte_carlo import MonteCarlo
    documents, words = _ap_text(ap_train, TRAIN["documents"])
    np.random.seed(numpy_seed)
    m = MonteCarlo(hyper_parameter_optimize_interval=TRAIN["interval"], seed=TRAIN["seed"] + seed_offset, blocks=TRAIN["blocks"], device=device,
                   process_group=group)
    m._verbose = False
    m._initialize(_shard_lines(documents, world, rank), words, TRAIN["topics"], 0.1, 1.0 / len(words))
    trace = [m.learning() for _ in range(TRAIN["iterations"])]
    n_kv, n_k, topics = m._counts(want_n_kv=True, want_topics=True)
    return dict(trace=np.array(trace), n_kv=n_kv, n_k=n_k, topics=topics, alpha=m._alpha_alpha, beta=m._alpha_beta,
                first=m._first_document)


def _monte_carlo_worker(rank, world, port, out_dir, backend):
    import datetime
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    device = rank if backend == "nccl" else 0
    torch.cuda.set_device(device)
    limit = datetime.timedelta(seconds=SPAWN_LIMIT // 2)
    if backend == "nccl":
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=limit, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=limit)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ap_train_k10.npz")))
    g["term_id"], g["term_ct"] = g["term_id"].astype(np.int32), g["term_ct"].astype(np.int32)
    # every rank but the first starts from another state of numpy's stream and is handed another sampler seed: the
    # engine has to install rank 0's of both
    out = _train(g, dist.group.WORLD, world, rank, device, numpy_seed=rank * 17, seed_offset=rank * 5)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def _assert_ranks_equal_one_process(ap_train, out_dir, world):
    single = _train(ap_train)
    ranks = [np.load(os.path.join(out_dir, "rank%d.npz" % r)) for r in range(world)]
    assert [int(r["first"]) for r in ranks] == [0, 170]
    assert np.array_equal(np.concatenate([r["topics"] for r in ranks]), single["topics"])
    for r in ranks:
        for name in ("n_kv", "n_k", "alpha", "beta"):
            assert np.array_equal(r[name], single[name]), name
        assert rel_err(r["trace"], single["trace"]) < 1e-12          # (only the order of the documents' sum differs)
        assert np.array_equal(r["trace"], ranks[0]["trace"])
    assert not np.array_equal(single["alpha"], np.full(TRAIN["topics"], 0.1))      # the hyper-parameter step moved


def test_two_ranks_on_one_gpu_train_the_one_process_chain(ap_train, tmp_path):
    _spawn(_monte_carlo_worker, (2, _free_port(), str(tmp_path), "gloo"), 2)
    _assert_ranks_equal_one_process(ap_train, str(tmp_path), 2)


def _gpu_count():
    try:
        from pylda_amd import _capi
        return _capi.device_count()
    except Exception:
        return 0


@pytest.mark.skipif(_gpu_count() < 2, reason="needs two GPUs: RCCL refuses two ranks on one device")
def test_two_gpus_over_rccl_train_the_one_process_chain(ap_train, tmp_path):
    _spawn(_monte_carlo_worker, (2, _free_port(), str(tmp_path), "nccl"), 2)
    _assert_ranks_equal_one_process(ap_train, str(tmp_path), 2)


@pytest.fixture
def nccl_world_of_one(monkeypatch):
    import torch
    import torch.distributed as dist
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_rccl_exchange_is_zero_copy_on_the_context_stream(ap_train, nccl_world_of_one, monkeypatch):
    """A world of one rank over RCCL: the sharded path (sample, all-gather on the library's buffers, apply of the
    gathered records) gives the one-process chain, and every all-gather is issued under the stream the kernels run on."""
    import torch
    import torch.distributed as dist
    seen = []
    real = dist.all_gather_into_tensor

    def spy(output, input, *args, **kwargs):
        seen.append((torch.cuda.current_stream().cuda_stream, output.data_ptr(), input.data_ptr(), input.numel()))
        return real(output, input, *args, **kwargs)
    monkeypatch.setattr(dist, "all_gather_into_tensor", spy)
    single = _train(ap_train)
    assert not seen
    from pylda_amd import monte_carlo
    contexts = []
    real_context = monte_carlo.MonteCarlo._context

    def remember(self):
        contexts.append(real_context(self))
        return contexts[-1]
    monkeypatch.setattr(monte_carlo.MonteCarlo, "_context", remember)
    sharded = _train(ap_train, nccl_world_of_one, 1, 0)
    for name in ("topics", "n_kv", "n_k", "alpha", "beta"):
        assert np.array_equal(sharded[name], single[name]), name
    assert rel_err(sharded["trace"], single["trace"]) < 1e-12
    stream = contexts[-1]._torch_stream.cuda_stream
    assert len(seen) == TRAIN["blocks"] * TRAIN["iterations"]
    assert set(s for s, _, _, _ in seen) == {stream} and stream != torch.cuda.default_stream().cuda_stream
    assert len(set((o, i) for _, o, i, _ in seen)) == 1 and seen[0][1] != seen[0][2]


# ---- the command line ----
def _write_corpus(ap_train, tmp_path, n_docs, blank_after_first=False):
    documents, words = _ap_text(ap_train, n_docs + 8)
    corpus_dir = tmp_path / "mini-press"
    corpus_dir.mkdir()
    train = documents[:n_docs]
    if blank_after_first:
        train = [train[0], ""] + train[1:]
    (corpus_dir / "train.dat").write_text("\n".join(train) + "\n")
    (corpus_dir / "test.dat").write_text("\n".join(documents[n_docs:]) + "\n")
    (corpus_dir / "voc.dat").write_text("".join("%s\t1\t1\n" % w for w in words))
    return corpus_dir


def _run_in_its_own_session(cmd, env, cwd):
    """subprocess.run under SPAWN_LIMIT whose time limit ends the launcher AND its ranks: the command leads a session of
    its own and the whole process group is killed (ranks stuck in a collective would outlive their launcher)."""
    import signal
    process = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=cwd,
                               start_new_session=True)
    try:
        out, err = process.communicate(timeout=SPAWN_LIMIT)
    except subprocess.TimeoutExpired:
        os.killpg(process.pid, signal.SIGKILL)
        out, err = process.communicate()
        pytest.fail("the command did not finish within %d s: %s\n%s" % (SPAWN_LIMIT, out[-2000:], err[-4000:]), pytrace=False)
    return subprocess.CompletedProcess(cmd, process.returncode, out, err)


def _launch_train(corpus_dir, out_dir, tmp_path, topics, iterations, interval, blocks, gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYLDA_SEED"] = "11"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "pylda_amd.launch_train", "--input_directory=%s/" % corpus_dir, "--output_directory=%s" % out_dir,
           "--number_of_topics=%d" % topics, "--training_iterations=%d" % iterations, "--snapshot_interval=%d" % interval,
           "--inference_mode=1", "--sampler_seed=4", "--gibbs_blocks=%d" % blocks]
    if gpus > 1:
        cmd += ["--gibbs_sharded=1", "--gpus=%d" % gpus, "--share_gpu=1"]
    done = _run_in_its_own_session(cmd, env, str(tmp_path))
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    found = list((out_dir / "mini-press").iterdir())
    assert len(found) == 1                                       # ONE run directory, rank 0's
    assert done.stdout.count("successfully load all training docs") == 1
    return found[0]


def _assert_same_run(one, many, iterations, interval, topics):
    for at in range(interval, iterations + 1, interval):
        assert (one / ("exp_gamma-%d" % at)).read_bytes() == (many / ("exp_gamma-%d" % at)).read_bytes(), at
        a, b = ((run / ("exp_beta-%d" % at)).read_text().split("==========\t") for run in (one, many))
        assert len(a) == len(b) == 1 + topics
        for block_a, block_b in zip(a, b):                       # topic by topic (words of equal probability: any order)
            assert sorted(block_a.splitlines()) == sorted(block_b.splitlines()), at
    models = [pickle.load(open(run / ("model-%d" % iterations), "rb")) for run in (one, many)]
    for x, y in zip(models[0]._host_state, models[1]._host_state):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    for x, y in zip(models[0]._train_csr, models[1]._train_csr):
        assert np.array_equal(x, y)
    assert models[1]._process_group is None and models[1]._ctx is None and models[1]._first_document == 0
    assert models[1]._counter == iterations and models[1]._number_of_documents == models[0]._number_of_documents
    assert np.array_equal(models[0]._alpha_alpha, models[1]._alpha_alpha) and np.array_equal(models[0]._alpha_beta, models[1]._alpha_beta)
    return models


def test_launch_train_sharded_over_two_ranks_writes_the_one_gpu_run(ap_train, tmp_path, capfd):
    from pylda_amd import cli
    corpus_dir = _write_corpus(ap_train, tmp_path, 150)
    runs = [_launch_train(corpus_dir, tmp_path / ("out%d" % gpus), tmp_path, 5, 10, 5, 16, gpus) for gpus in (1, 2)]
    one, two = _assert_same_run(runs[0], runs[1], 10, 5, 5)
    assert two._number_of_documents == 150
    likelihoods = []
    for run in runs:                                             # the snapshot is an ordinary mode-1 snapshot
        capfd.readouterr()
        assert cli.test_main(["--input_directory=%s" % corpus_dir, "--model_directory=%s" % run, "--fold_in_samples=20"]) == 0
        lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("held-out likelihood of snapshot")]
        assert len(lines) == 1
        likelihoods.append(lines[0].split(" is ")[1])
    assert likelihoods[0] == likelihoods[1]
    assert one.learning() == two.learning()                      # ... the same chain from either snapshot


def test_launch_train_sharded_with_more_ranks_than_documents(ap_train, tmp_path):
    """Three ranks, two documents and an empty line between them: one rank holds no document and still joins every
    collective of every round."""
    corpus_dir = _write_corpus(ap_train, tmp_path, 2, blank_after_first=True)
    runs = [_launch_train(corpus_dir, tmp_path / ("out%d" % gpus), tmp_path, 4, 6, 3, 16, gpus) for gpus in (1, 3)]
    one, three = _assert_same_run(runs[0], runs[1], 6, 3, 4)
    assert three._number_of_documents == 2
