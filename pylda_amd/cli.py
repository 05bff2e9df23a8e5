"""Command-line drivers that speak the reference's launch_train / launch_test
interface (flags, output directory layout, snapshot files) on top of the
MI355X variational-Bayes engine.

Behavioural contract taken from the reference:
  training   launch_train.py:31-62 (flags), :102-115 (corpus files), :119-124 (default
             priors), :127-141 (run directory name), :148-162 (option.txt), :196-204
             (snapshot cadence, exp_beta-N / exp_gamma-N / model-N)
  held-out   launch_test.py:18-23 (flags), :49-57 (corpus-name check), :62-66 (test.dat),
             :90-97 (per-snapshot evaluation, test-N via numpy.savetxt)
Inference mode 2 (variational Bayes) is the default engine here.  Mode 0 (hybrid, hybrid.py) runs with
--sampler_seed=N: its sampler draws from a counter-based stream that no numpy seed can reproduce, so it is run only
when asked for by that flag, never in place of a reference run.  Mode 1 (collapsed Gibbs, monte_carlo.py) runs with
--sampler_seed=N --gibbs_blocks=G: a document-parallel approximation of the reference's sequential chain, G rounds per
sweep (pylda_amd/monte_carlo.py); without --gibbs_blocks it is refused.  Mode 3 (collapsed variational Bayes in its
zero-order form, CVB0; pylda_amd/cvb0.py), which the reference does not have, runs with --sampler_seed=N --cvb0_blocks=G on
one GPU: deterministic after its start, G rounds per sweep; its snapshot answers launch_test as a mode-2 snapshot does.
With --cvb0_minibatches=B in place of --cvb0_blocks it is the stochastic form (SCVB0; pylda_amd/scvb0.py), which keeps no state
per token: an iteration is then one epoch of B minibatch steps ([--cvb0_burn_in=P] burn-in passes per document,
[--cvb0_tau0=T] [--cvb0_kappa=K] the step sizes), on one GPU, and the snapshot answers launch_test the same way.  Mode 1 on
several GPUs (--gpus N) runs only with
--gibbs_sharded=1: every rank then holds a range of the documents and a replica of the whole word-topic table, and the
ranks exchange the block's topic changes in every round - G collectives per sweep - which gives the one-GPU run's topics
on every token; the snapshot is an ordinary one-process mode-1 snapshot.  A mode-1 snapshot is evaluated by launch_test
--fold_in_samples=S: held-out fold-in against its frozen counts.  Mode 2 with --online_batches=B is online variational
Bayes (pylda_amd/online_vb.py), which the reference does not have: an iteration is then one step on one of B minibatches,
on one GPU, and the snapshot answers launch_test as a mode-2 snapshot does.  launch_test --document_completion=1 reports
the document-completion likelihood of a snapshot of any engine instead of the plug-in figure (a mode-1 snapshot with
--fold_in_samples=S): theta from one half of every test document, the other half scored, per-word perplexity.
launch_test --left_to_right=R reports the left-to-right likelihood of a snapshot of any engine - log p(w) of the whole test
documents with theta integrated out, R particles a document - in place of the plug-in figure; no theta is fitted.
launch_test --topic_coherence=M scores the topics of every snapshot first: UMass and NPMI coherence of each topic's top M
words, counted over the documents of test.dat (coherence-N beside test-N).
launch_test --similar_documents=N finds, from the test gamma of every snapshot, the N nearest training documents of every test
document by Hellinger distance between topic mixtures (similar-N beside test-N).
launch_test --similar_topics=N finds the N nearest other topics of every topic of a snapshot by Jensen-Shannon distance between
the topics' word distributions (similar-topics-N), and --topic_match=DIR matches the topics of snapshot model-N one to one with
those of DIR/model-N, a run of any engine over the same vocabulary (match-N); both run where --topic_coherence runs.
"""
import argparse
import datetime
import os
import pickle
import sys

import numpy

TRAIN_FLAGS = (
    # name, type, default, help
    ("input_directory", str, None, "input directory [None]"),
    ("output_directory", str, None, "output directory [None]"),
    ("number_of_topics", int, -1, "total number of topics [-1]"),
    ("training_iterations", int, -1, "total number of iterations [-1]"),
    ("snapshot_interval", int, 10, "snapshot interval [10]"),
    ("alpha_alpha", float, -1, "hyper-parameter for Dirichlet distribution of topics [1.0/number_of_topics]"),
    ("alpha_beta", float, -1, "hyper-parameter for Dirichlet distribution of vocabulary [1.0/number_of_types]"),
    ("inference_mode", int, 2, "inference mode [2: variational bayes; 0: hybrid, with --sampler_seed; 1: collapsed Gibbs, "
                               "with --sampler_seed and --gibbs_blocks; 3: collapsed variational Bayes (CVB0), with "
                               "--sampler_seed and --cvb0_blocks]"),
    ("sampler_seed", int, -1, "seed of the samplers' counter-based random numbers [-1: none; "
                              "--inference_mode=0, 1 and 3 need one]"),
    ("gibbs_blocks", int, -1, "rounds per sweep of the collapsed Gibbs engine [-1: none; --inference_mode=1 needs one]: the "
                              "documents with index g modulo G are sampled together in round g; the more rounds, the closer "
                              "to the reference's sequential chain"),
    ("cvb0_blocks", int, -1, "rounds per sweep of the collapsed variational Bayes engine [-1: none; --inference_mode=3 needs "
                             "one]: the documents with index g modulo G are updated together in round g; G >= the number of "
                             "documents is sequential CVB0"),
    ("cvb0_minibatches", int, -1, "stochastic collapsed variational Bayes, SCVB0 [-1: off; with --inference_mode=3 and "
                                  "--sampler_seed, in place of --cvb0_blocks, on one GPU only]: B minibatches, the documents "
                                  "with index b modulo B form minibatch b; an iteration is one epoch of B steps"),
    ("cvb0_burn_in", int, None, "burn-in passes over a document before the pass that counts, per visit [1]; 0 to 15"),
    ("cvb0_tau0", float, None, "delay of SCVB0's step sizes (tau0 + t) ** (-kappa), of the topics and of the documents [10.0]; "
                             "at least 1"),
    ("cvb0_kappa", float, None, "forgetting rate of SCVB0's step sizes [0.9]; above 0.5, at most 1"),
    ("gibbs_sharded", int, 0, "collapsed Gibbs over --gpus N [0: refused]: 1 = every rank holds a range of the documents and a "
                              "replica of the whole word-topic table (4 bytes x types x topics per GPU), and the ranks exchange "
                              "the block's topic changes in each of the G rounds of a sweep (G collectives per sweep)"),
    ("online_batches", int, -1, "online variational Bayes [-1: off; with --inference_mode=2 on one GPU only]: B minibatches, "
                                "the documents with index b modulo B form minibatch b; --training_iterations and "
                                "--snapshot_interval then count minibatch steps, and alpha stays fixed"),
    ("online_tau0", float, -1, "delay of the online step size rho_t = (tau0 + t) ** (-kappa) [1.0]; at least 1"),
    ("online_kappa", float, -1, "forgetting rate of the online step size [0.7]; above 0.5, at most 1"),
    ("device", int, 0, "GPU index [0] (one process; with --gpus N rank r runs on GPU r)"),
    ("gpus", int, 1, "GPUs of this node to shard the documents over [1]: re-executes itself under "
                     "torch.distributed.run, one rank per GPU, one RCCL all-reduce of the K x V statistics per iteration"),
    ("share_gpu", int, 0, "test mode [0]: 1 = all ranks on GPU 0, exchange over gloo (RCCL refuses two ranks per device)"),
)
TEST_FLAGS = (
    ("input_directory", str, None, "input directory [None]"),
    ("model_directory", str, None, "model directory [None]"),
    ("snapshot_index", int, -1, "snapshot index [-: evaluate on all available snapshots]"),
    ("fold_in_samples", int, -1, "sweeps of the held-out fold-in [-1: off; a collapsed Gibbs (mode 1) snapshot needs it]: the "
                                 "engine's fold_in() is called in place of inference()"),
    ("fold_in_burn_in", int, -1, "sweeps of the fold-in left out of the average [fold_in_samples // 2]"),
    ("document_completion", int, 0, "[0] 1 = the document-completion likelihood: theta is fitted on one half of every test "
                                    "document (the tokens at even positions), the other half is scored, per-word perplexity is "
                                    "reported; test-N holds the observed halves' gamma"),
    ("left_to_right", int, 0, "[0: off] R = the left-to-right held-out likelihood (Wallach et al. 2009) with R particles per "
                              "document (1 .. 256): log p(w) with theta integrated out, per-word perplexity; it evaluates the "
                              "model alone, fits no theta and writes no test-N; a mode-1 snapshot needs no --fold_in_samples"),
    ("left_to_right_resample", int, 1, "[1] 0 = the sequential sampler (a step per token), 1 = every earlier token of the "
                                       "document drawn again before each token (Algorithm 3)"),
    ("topic_coherence", int, 0, "[0: off] M = UMass and NPMI coherence of every topic's top M words (1 .. 64), counted over the "
                                "documents of test.dat; coherence-N holds a line per topic: index, UMass, NPMI, the words"),
    ("similar_documents", int, 0, "[0: off] N = the N nearest training documents of every test document by Hellinger distance "
                                  "between topic mixtures (1 .. 64); similar-N holds a line per test document: id:distance, "
                                  "separated by tabs, nearest first"),
    ("similar_topics", int, 0, "[0: off] N = the N nearest other topics of every topic by Jensen-Shannon distance between the "
                               "topics' word distributions (1 .. 64); similar-topics-N holds a line per topic: id:distance, "
                               "separated by tabs, nearest first"),
    ("topic_match", str, None, "[None: off] DIR = a model directory of the same corpus: the topics of snapshot model-N are matched "
                               "one to one with those of DIR/model-N by Jensen-Shannon distance; match-N holds a line per "
                               "topic: index, matched index (-1: none), distance, five top words of each"),
)
RULE = "========== ========== ========== ========== =========="


def _parse(flags, argv, prog):
    parser = argparse.ArgumentParser(prog=prog, allow_abbrev=False)
    for name, kind, default, text in flags:
        parser.add_argument("--" + name, type=kind, default=default, help=text)
    return parser.parse_args(argv)


def _lines(path):
    with open(path, "r") as stream:
        return [line.strip().lower() for line in stream]


def _phase(label, since):
    """PYLDA_TIMING=1: wall time of the start-up phases on stderr (every rank)."""
    import time
    now = time.perf_counter()
    if os.environ.get("PYLDA_TIMING"):
        sys.stderr.write("[pylda timing] rank %s %-40s %8.1f ms\n" % (os.environ.get("RANK", "0"), label, (now - since) * 1e3))
    return now


def _banner(pairs):
    print(RULE)
    for key, value in pairs:
        print("%s=%s" % (key, value))
    print(RULE)


def train_main(argv=None):
    opt = _parse(TRAIN_FLAGS, argv, "launch_train")
    for required in ("number_of_topics", "training_iterations", "snapshot_interval"):
        if getattr(opt, required) <= 0:
            raise SystemExit("--%s must be positive" % required)
    if opt.input_directory is None or opt.output_directory is None:
        raise SystemExit("--input_directory and --output_directory are required")
    online = opt.online_batches != -1
    if not online and (opt.online_tau0 != -1 or opt.online_kappa != -1):
        sys.stderr.write("error: --online_tau0 and --online_kappa set the step size of online variational Bayes, which runs "
                         "with --online_batches=B only...\n")
        return 2
    if online:
        refusal = _online_refusal(opt)
        if refusal:
            sys.stderr.write("error: %s...\n" % refusal)
            return 2
    hybrid = opt.inference_mode == 0 and opt.sampler_seed >= 0
    if opt.inference_mode == 0 and not hybrid:
        sys.stderr.write("error: inference mode 0 (hybrid) needs --sampler_seed=N: its sampler draws from a counter-based "
                         "random stream (Philox), which cannot reproduce a numpy-seeded reference run - pass the flag to "
                         "run it anyway...\n")
        return 2
    gibbs = opt.inference_mode == 1 and opt.sampler_seed >= 0 and opt.gibbs_blocks >= 1
    if opt.inference_mode == 1 and not gibbs:
        sys.stderr.write("error: inference mode 1 (collapsed Gibbs) needs --sampler_seed=N and --gibbs_blocks=G (G >= 1): what "
                         "runs here is a document-parallel approximation of the reference's sequential chain - G rounds per "
                         "sweep, the documents of a round sampled together against the counts of the round's start; the "
                         "more rounds, the closer to the reference (G >= the number of documents is its sampler) - pass both "
                         "flags to run it...\n")
        return 2
    if gibbs and (opt.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1) and opt.gibbs_sharded != 1:
        sys.stderr.write("error: inference mode 1 (collapsed Gibbs) runs on one GPU, got --gpus=%d; pass --gibbs_sharded=1 to "
                         "shard its documents over the GPUs: every rank then keeps a replica of the whole word-topic table "
                         "and the ranks exchange the topic changes in every round, --gibbs_blocks collectives per sweep...\n"
                         % opt.gpus)
        return 2
    stochastic = opt.cvb0_minibatches != -1
    if not stochastic and (opt.cvb0_burn_in is not None or opt.cvb0_tau0 is not None or opt.cvb0_kappa is not None):
        sys.stderr.write("error: --cvb0_burn_in, --cvb0_tau0 and --cvb0_kappa set the schedule of stochastic collapsed "
                         "variational Bayes, which runs with --cvb0_minibatches=B only...\n")
        return 2
    if stochastic:
        refusal = _stochastic_refusal(opt)
        if refusal:
            sys.stderr.write("error: %s...\n" % refusal)
            return 2
    cvb0 = opt.inference_mode == 3 and opt.sampler_seed >= 0 and (opt.cvb0_blocks >= 1 or stochastic)
    if opt.inference_mode == 3 and not cvb0:
        sys.stderr.write("error: inference mode 3 (collapsed variational Bayes, CVB0) needs --sampler_seed=N and "
                         "--cvb0_blocks=G (G >= 1): the reference has no such engine; its start draws from a counter-based "
                         "random stream, and what runs here is a document-parallel form of the chain - G rounds per sweep, "
                         "the documents of a round updated together against the expected counts of the round's start (G >= "
                         "the number of documents is sequential CVB0) - pass both flags to run it...\n")
        return 2
    if cvb0 and (opt.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        sys.stderr.write("error: inference mode 3 (collapsed variational Bayes) runs on one GPU, got --gpus=%d "
                         "(WORLD_SIZE=%s): sharding it over several GPUs is not built...\n"
                         % (opt.gpus, os.environ.get("WORLD_SIZE", "1")))
        return 2
    if opt.inference_mode not in (1, 2) and not hybrid and not cvb0:
        sys.stderr.write("error: pylda_amd implements inference modes 2 (variational bayes), 0 (hybrid, with "
                         "--sampler_seed), 1 (collapsed Gibbs, with --sampler_seed and --gibbs_blocks) and 3 (collapsed "
                         "variational Bayes, with --sampler_seed and --cvb0_blocks), got %d...\n"
                         % opt.inference_mode)
        return 2
    if opt.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # invoked as the reference's one-process command: become the launcher, one rank per GPU
        os.execv(sys.executable, _launcher_argv(opt.gpus, sys.argv[1:] if argv is None else list(argv)))
    rank, world, device, group = _join_ranks(opt)
    seed = os.environ.get("PYLDA_SEED")      # the reference has no seed flag (numpy's global RNG, unseeded): reproducible runs
    if rank != 0:
        sys.stdout = open(os.devnull, "w")    # one copy of the reference's console output
    source = opt.input_directory.rstrip("/")
    corpus_name = os.path.basename(source)
    documents = _lines(os.path.join(source, "train.dat"))
    print("successfully load all training docs from %s..." % os.path.abspath(os.path.join(source, "train.dat")))
    if stochastic and opt.cvb0_minibatches > len(documents):
        sys.stderr.write("error: --cvb0_minibatches=%d exceeds the %d documents of %s: a minibatch would be empty...\n"
                         % (opt.cvb0_minibatches, len(documents), os.path.abspath(os.path.join(source, "train.dat"))))
        return 2
    if online and opt.online_batches > len(documents):
        sys.stderr.write("error: --online_batches=%d exceeds the %d documents of %s: a minibatch would be empty...\n"
                         % (opt.online_batches, len(documents), os.path.abspath(os.path.join(source, "train.dat"))))
        return 2
    vocabulary = list(dict.fromkeys(entry.split()[0] for entry in _lines(os.path.join(source, "voc.dat")) if entry))
    print("successfully load all the words from %s..." % os.path.abspath(os.path.join(source, "voc.dat")))
    topics = opt.number_of_topics
    prior_topics = opt.alpha_alpha if opt.alpha_alpha > 0 else 1.0 / topics
    prior_words = opt.alpha_beta if opt.alpha_beta > 0 else 1.0 / len(vocabulary)

    stamp = datetime.datetime.now().strftime("%y%m%d-%H%M%S")
    run = "%s-lda-I%d-S%d-K%d-aa%f-ab%f-im%d/" % (stamp, opt.training_iterations, opt.snapshot_interval,
                                                  topics, prior_topics, prior_words, opt.inference_mode)
    run_dir = os.path.join(opt.output_directory, corpus_name, run)
    if rank == 0:
        os.makedirs(os.path.abspath(run_dir))
    settings = (("input_directory", source), ("corpus_name", corpus_name),
                ("training_iterations", "%d" % opt.training_iterations),
                ("snapshot_interval", str(opt.snapshot_interval)), ("number_of_topics", str(topics)),
                ("alpha_alpha", str(prior_topics)), ("alpha_beta", str(prior_words)),
                ("inference_mode", "%d" % opt.inference_mode))
    if hybrid or gibbs or cvb0:
        settings += (("sampler_seed", "%d" % opt.sampler_seed),)
    if gibbs:
        settings += (("gibbs_blocks", "%d" % opt.gibbs_blocks),)
    if stochastic:
        settings += (("cvb0_minibatches", "%d" % opt.cvb0_minibatches), ("cvb0_burn_in", "%d" % opt.cvb0_burn_in),
                     ("cvb0_tau0", str(opt.cvb0_tau0)), ("cvb0_kappa", str(opt.cvb0_kappa)))
    elif cvb0:
        settings += (("cvb0_blocks", "%d" % opt.cvb0_blocks),)
    if online:
        settings += (("online_batches", "%d" % opt.online_batches), ("online_tau0", str(opt.online_tau0)),
                     ("online_kappa", str(opt.online_kappa)))
    if rank == 0:
        with open(run_dir + "option.txt", "w") as out:
            out.writelines("%s=%s\n" % pair for pair in settings)
    _banner((("output_directory", run_dir),) + settings[:1] + settings[1:])

    from pylda_amd.variational_bayes import VariationalBayes
    import time
    if hybrid:
        from pylda_amd.hybrid import Hybrid
        engine = Hybrid(device=device, process_group=group, seed=opt.sampler_seed)
    elif gibbs:
        from pylda_amd.monte_carlo import MonteCarlo
        engine = MonteCarlo(device=device, seed=opt.sampler_seed, blocks=opt.gibbs_blocks, process_group=group)
    elif stochastic:
        from pylda_amd.scvb0 import StochasticCollapsedVariationalBayes
        engine = StochasticCollapsedVariationalBayes(opt.cvb0_minibatches, burn_in=opt.cvb0_burn_in, tau0=opt.cvb0_tau0,
                                                     kappa=opt.cvb0_kappa, theta_tau0=opt.cvb0_tau0, theta_kappa=opt.cvb0_kappa,
                                                     device=device, seed=opt.sampler_seed)
    elif cvb0:
        from pylda_amd.cvb0 import CollapsedVariationalBayes
        engine = CollapsedVariationalBayes(device=device, seed=opt.sampler_seed, blocks=opt.cvb0_blocks)
    elif online:
        from pylda_amd.online_vb import OnlineVariationalBayes
        engine = OnlineVariationalBayes(opt.online_batches, tau0=opt.online_tau0, kappa=opt.online_kappa, device=device)
    else:
        engine = VariationalBayes(device=device, process_group=group)
    if seed is not None:
        numpy.random.seed(int(seed))
    started = time.perf_counter()
    if online or stochastic:
        try:
            engine._initialize(documents, vocabulary, topics, prior_topics, prior_words)
        except ValueError as refused:       # (documents the vocabulary leaves empty are dropped: fewer than there are lines)
            sys.stderr.write("error: --%s: %s...\n" % ("online_batches" if online else "cvb0_minibatches", refused))
            return 2
    elif group is None:
        engine._initialize(documents, vocabulary, topics, prior_topics, prior_words)
    elif gibbs:
        _initialize_gibbs_shard(engine, documents, vocabulary, topics, prior_topics, prior_words, rank, world)
    else:
        _initialize_shard(engine, documents, vocabulary, topics, prior_topics, prior_words, rank, world)
    _phase("parse + initial eta", started)
    whole, whole_at = None, -1
    for _ in range(opt.training_iterations):
        engine.learning()
        if engine._counter % opt.snapshot_interval == 0:
            whole, whole_at = _whole_model(engine, group, rank, world), engine._counter
            if rank == 0:
                whole.export_beta("%sexp_beta-%d" % (run_dir, engine._counter))
                whole.export_gamma("%sexp_gamma-%d" % (run_dir, engine._counter))
    # (the last iteration's exports already gathered gamma - 2 GB at cfg 4: the snapshot adds the corpus to that copy)
    whole = _whole_model(engine, group, rank, world, with_corpus=True, reuse_gamma=whole_at == engine._counter, gathered=whole)
    if rank == 0:
        with open(os.path.join(run_dir, "model-%d" % engine._counter), "wb") as out:
            pickle.dump(whole, out)
    if group is not None:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


def _online_refusal(opt):
    """Why --online_batches cannot run with the other flags (None: it can); fills in the step size's defaults."""
    from pylda_amd.online_vb import check_schedule
    if opt.inference_mode != 2:
        return ("--online_batches is online variational Bayes and runs with --inference_mode=2 only, got "
                "--inference_mode=%d: the engines of modes 0, 1 and 3 have no minibatch form here" % opt.inference_mode)
    if opt.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return ("--online_batches runs on one GPU, got --gpus=%d (WORLD_SIZE=%s): sharding the minibatches over several "
                "GPUs is not built" % (opt.gpus, os.environ.get("WORLD_SIZE", "1")))
    if opt.online_tau0 == -1:
        opt.online_tau0 = 1.0
    if opt.online_kappa == -1:
        opt.online_kappa = 0.7
    try:
        check_schedule(opt.online_batches, opt.online_tau0, opt.online_kappa)
    except ValueError as refused:
        return "--online_batches / --online_tau0 / --online_kappa: %s" % refused
    return None


def _stochastic_refusal(opt):
    """Why --cvb0_minibatches cannot run with the other flags (None: it can); fills in the schedule's defaults."""
    from pylda_amd.online_vb import check_schedule
    from pylda_amd.scvb0 import check_burn_in
    if opt.inference_mode != 3:
        return ("--cvb0_minibatches is stochastic collapsed variational Bayes and runs with --inference_mode=3 only, got "
                "--inference_mode=%d" % opt.inference_mode)
    if opt.cvb0_blocks != -1:
        return ("--cvb0_minibatches=%d and --cvb0_blocks=%d name two engines: the stochastic form deals the documents into "
                "minibatches itself and takes no --cvb0_blocks" % (opt.cvb0_minibatches, opt.cvb0_blocks))
    if opt.sampler_seed < 0:
        return "--cvb0_minibatches needs --sampler_seed=N: the start draws from a counter-based random stream"
    if opt.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return ("--cvb0_minibatches runs on one GPU, got --gpus=%d (WORLD_SIZE=%s): sharding the minibatches over several "
                "GPUs is not built" % (opt.gpus, os.environ.get("WORLD_SIZE", "1")))
    if opt.cvb0_burn_in is None:
        opt.cvb0_burn_in = 1
    if opt.cvb0_tau0 is None:
        opt.cvb0_tau0 = 10.0
    if opt.cvb0_kappa is None:
        opt.cvb0_kappa = 0.9
    try:
        check_schedule(opt.cvb0_minibatches, opt.cvb0_tau0, opt.cvb0_kappa)
        check_burn_in(opt.cvb0_burn_in)
    except ValueError as refused:
        return "--cvb0_minibatches / --cvb0_burn_in / --cvb0_tau0 / --cvb0_kappa: %s" % refused
    return None


def _launcher_argv(gpus, argv):
    """`python -m pylda_amd.launch_train ... --gpus N` as N ranks of this node (rendezvous on 127.0.0.1)."""
    import socket
    probe = socket.socket()
    probe.bind(("127.0.0.1", 0))
    port = probe.getsockname()[1]
    probe.close()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "pylda_amd.launch_train"] + list(argv)


def _join_ranks(opt):
    """(rank, world, device, process group) of a --gpus N run; (0, 1, --device, None) otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and opt.gpus <= 1:
        # started under torchrun (or another launcher) without --gpus: WORLD_SIZE ranks that each trained the whole
        # corpus on --device and wrote the same run directory would be silently wrong - the launcher's size it is
        opt.gpus = world
    if "WORLD_SIZE" in os.environ and opt.gpus != world:
        # (also --gpus 4 under a launcher of ONE rank: a quarter of the machine silently doing all of the work)
        raise SystemExit("--gpus %d does not match the launcher's WORLD_SIZE %d" % (opt.gpus, world))
    if opt.gpus <= 1 or world <= 1:
        return 0, 1, opt.device, None
    import torch
    import torch.distributed as dist
    if "RANK" not in os.environ:
        raise SystemExit("WORLD_SIZE=%d is set but RANK is not: start the ranks with torch.distributed.run (or pass "
                         "--gpus N and let launch_train start them)" % world)
    rank = int(os.environ["RANK"])
    device = 0 if opt.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(device)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if opt.share_gpu:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    return rank, world, device, dist.group.WORLD


def _host_group():
    """A gloo group next to the RCCL one, for the host-side object exchanges (eta of the start, gamma for exports)."""
    import torch.distributed as dist
    if dist.get_backend() == "gloo":
        return dist.group.WORLD
    if not hasattr(_host_group, "group"):
        _host_group.group = dist.new_group(backend="gloo")
    return _host_group.group


def _line_ranges(documents, world):
    """Contiguous ranges of the corpus' lines, one per rank, balanced by TOKENS (blank-separated fields: the proxy for
    distinct terms that is known before parsing - SURVEY 8e balances by nnz, which needs the vocabulary look-up; bytes,
    the round-5 proxy, also weigh long words): world + 1 line offsets, the same on every rank."""
    weight = numpy.fromiter((line.count(" ") + 1 for line in documents), dtype=numpy.int64, count=len(documents))
    ends = numpy.cumsum(weight)
    total = int(ends[-1]) if len(ends) else 0
    bounds = [0]
    for r in range(1, world):
        at = int(numpy.searchsorted(ends, total * r / world, side="left"))
        bounds.append(min(max(at, bounds[-1]), len(documents)))
    bounds.append(len(documents))
    return bounds


def _initialize_shard(engine, documents, vocabulary, topics, prior_topics, prior_words, rank, world):
    """variational_bayes.py:82-96 on one rank of several: this rank parses ITS lines only (round 4 parsed the whole
    corpus on every rank and threw 1 - 1/N of it away), rank 0 alone draws eta (:95, the process' first draw from
    numpy's global stream - the reference's own initial state under a seed) and every rank receives it."""
    import torch
    import torch.distributed as dist
    from pylda_amd.inferencer import Inferencer
    lo, hi = _line_ranges(documents, world)[rank:rank + 2]
    Inferencer._initialize(engine, vocabulary, topics, prior_topics, prior_words)
    engine._parsed_corpus = None
    verbose, engine._verbose = engine._verbose, False
    engine._train_csr = engine.parse_to_csr(documents[lo:hi])
    engine._verbose = verbose
    engine._number_of_documents = len(engine._train_csr[0]) - 1
    parsed = torch.tensor([engine._number_of_documents], dtype=torch.int64)
    dist.all_reduce(parsed, group=_host_group())
    if verbose and rank == 0:       # the reference's line (variational_bayes.py:128) with the CORPUS' count, once
        print("successfully parse %d documents..." % int(parsed))
    engine._gamma = None
    engine._gamma_init_pending = True
    shape = (engine._number_of_topics, engine._number_of_types)
    eta = torch.from_numpy(numpy.random.gamma(100., 1. / 100., shape)) if rank == 0 else torch.empty(shape, dtype=torch.float64)
    dist.broadcast(eta, src=0, group=_host_group())
    engine._eta = eta.numpy()
    engine._ctx = None
    engine._train_corpus = None
    if hasattr(engine, "_first_document"):      # Hybrid: the sampler's streams are named by the GLOBAL document index
        engine._first_document = _shard_offset(engine._number_of_documents, rank, world)


def _initialize_gibbs_shard(engine, documents, vocabulary, topics, prior_topics, prior_words, rank, world):
    """monte_carlo.py:45-74 on one rank of several: this rank parses ITS lines only; the engine then finds its offset among
    the PARSED documents (lines the vocabulary leaves empty are dropped, as in a one-process run), draws its tokens'
    first topics under their global names and joins the sum of the ranks' count tables."""
    from pylda_amd.inferencer import Inferencer
    lo, hi = _line_ranges(documents, world)[rank:rank + 2]
    Inferencer._initialize(engine, vocabulary, topics, prior_topics, prior_words)
    verbose, engine._verbose = engine._verbose, False
    engine._parsed_corpus = engine.parse_data(documents[lo:hi])
    engine._verbose = verbose
    engine._initialize_parsed()
    if verbose and rank == 0:       # the reference's line (monte_carlo.py:100) with the CORPUS' count, once
        print("successfully parse %d documents..." % engine._global_documents)


def _shard_offset(local_documents, rank, world):
    """Documents on the ranks before this one (the shards are contiguous ranges of the corpus)."""
    import torch
    import torch.distributed as dist
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([local_documents], dtype=torch.int64), group=_host_group())
    return int(sum(int(t) for t in sizes[:rank]))


def _gather_rows(local, rank, world):
    """The ranks' arrays (equal trailing shape) one after the other in a pre-allocated array on rank 0 - tensor
    receives straight into its slices, no pickling (gamma is 2 GB at cfg 4); None elsewhere."""
    import torch
    import torch.distributed as dist
    group = _host_group()
    local = numpy.ascontiguousarray(local)
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([local.shape[0]], dtype=torch.int64), group=group)
    sizes = [int(t) for t in sizes]
    if rank != 0:
        if local.shape[0]:
            dist.send(torch.from_numpy(local), dst=0, group=group)
        return None
    whole = numpy.empty((sum(sizes),) + local.shape[1:], dtype=local.dtype)
    whole[:sizes[0]] = local
    at = sizes[0]
    for src in range(1, world):
        if sizes[src]:
            dist.recv(torch.from_numpy(whole[at:at + sizes[src]]), src=src, group=group)
        at += sizes[src]
    return whole


def _whole_model(engine, group, rank, world, with_corpus=False, reuse_gamma=False, gathered=None):
    """The engine the exporters and the snapshot pickle see: at one rank the engine itself; at several, on rank 0, a
    copy that holds the gamma rows of every rank in document order (the shards are contiguous) and - for the snapshot,
    which like the reference's pickle carries the parsed corpus - the whole corpus, gathered once.  reuse_gamma (the
    same on every rank): `gathered` is what this function returned for an export of the SAME iteration - rank 0 takes
    its gamma from there, only the corpus travels."""
    if group is None:
        return engine
    import copy
    from pylda_amd.monte_carlo import MonteCarlo
    if isinstance(engine, MonteCarlo):
        return gathered if reuse_gamma else _whole_gibbs_model(engine, rank, world)
    if reuse_gamma:
        gamma = gathered._gamma_host if rank == 0 else None
    else:
        gamma = _gather_rows(numpy.asarray(engine._gamma), rank, world)
    corpus = None
    if with_corpus:
        doc_ptr, term_id, term_ct = engine._train_csr
        lengths = _gather_rows(numpy.diff(numpy.asarray(doc_ptr, dtype=numpy.int64)), rank, world)
        ids = _gather_rows(numpy.asarray(term_id, dtype=numpy.int32), rank, world)
        cts = _gather_rows(numpy.asarray(term_ct, dtype=numpy.int32), rank, world)
        if rank == 0:
            corpus = (numpy.concatenate([numpy.zeros(1, numpy.int64), numpy.cumsum(lengths)]), ids, cts)
    if rank != 0:
        return None
    whole = copy.copy(engine)
    whole.__dict__.update(engine.__getstate__())          # host copies only, no device handles
    whole._gamma_host = gamma
    whole._train_csr = corpus
    whole._parsed_lists = None
    whole._number_of_documents = gamma.shape[0]
    return whole


def _whole_gibbs_model(engine, rank, world):
    """MonteCarlo over several ranks as the one-process engine it equals: on rank 0 a copy whose host state holds the
    corpus and the topics of every rank in document order (the shards are contiguous) and the word-topic counts and n_k
    of rank 0's replica (every replica holds the corpus').  Its exports count n_dk from the topics on the host; pickled, it
    is an ordinary mode-1 snapshot.  None on the other ranks."""
    doc_ptr, term_id, term_ct = engine._train_csr
    n_kv, n_k, topics = engine._counts(want_n_kv=rank == 0, want_topics=True)
    lengths = _gather_rows(numpy.diff(numpy.asarray(doc_ptr, dtype=numpy.int64)), rank, world)
    ids = _gather_rows(numpy.asarray(term_id, dtype=numpy.int32), rank, world)
    cts = _gather_rows(numpy.asarray(term_ct, dtype=numpy.int32), rank, world)
    topics = _gather_rows(numpy.asarray(topics, dtype=numpy.int32), rank, world)
    if rank != 0:
        return None
    whole = engine.__class__.__new__(engine.__class__)   # (not copy.copy: __getstate__ would read the counts back once more)
    state = dict(engine.__dict__)
    state.update(_ctx=None, _train_corpus=None, _process_group=None, _exchange=None, _parsed_corpus=None, _first_document=0,
                 _host_state=(n_kv, n_k, topics), _number_of_documents=len(lengths),
                 _train_csr=(numpy.concatenate([numpy.zeros(1, numpy.int64), numpy.cumsum(lengths)]), ids, cts))
    whole.__dict__.update(state)
    return whole


NEEDS_FOLD_IN_SAMPLES = "needs --fold_in_samples"     # evaluate_snapshot's answer for a fold-in engine asked without sweeps
NO_TRAINING_ROWS = "no training rows"                 # ... for similar documents asked of a snapshot that holds no training gamma
TOPIC_MATCH_MISSING = "no snapshot to match"          # ... for --topic_match where DIR holds no snapshot of that index
TOPIC_MATCH_VOCABULARY = "another vocabulary"         # ... (with the difference, as a pair) where its vocabulary is another


def report_similar_documents(engine, snapshot_path, gamma, similar_path, top):
    """The `top` nearest training documents of every test document (its row of `gamma`) by Hellinger distance: one line on
    stdout, a line per test document in similar_path.  False: the snapshot holds no rows of its training documents."""
    try:
        result = engine.similar_documents(numpy.asarray(gamma, dtype=numpy.float64), top)
    except RuntimeError as error:
        if "no rows of its training documents" not in str(error):
            raise
        return False
    nearest = result.distance[:, 0] if len(result.distance) else numpy.zeros(0)
    print("similar documents of snapshot %s: the %d nearest of %d training documents for %d test documents, mean nearest "
          "Hellinger distance %g" % (os.path.abspath(snapshot_path), top, result.documents, len(result.ids),
                                     float(numpy.mean(nearest)) if len(nearest) else numpy.nan))
    with open(similar_path, "w") as output:
        for ids, distances in zip(result.ids, result.distance):
            output.write("\t".join("%d:%.17g" % (d, x) for d, x in zip(ids, distances) if d >= 0) + "\n")
    return True


TOPIC_METRIC = "jensen_shannon"       # the metric of --similar_topics and --topic_match


def report_similar_topics(engine, snapshot_path, similar_path, top):
    """The `top` nearest other topics of every topic of the snapshot: one line on stdout, a line per topic in similar_path."""
    result = engine.topic_distances(None, TOPIC_METRIC)
    ids, distances = result.nearest(top)
    if ids.shape[1]:
        k = int(numpy.argmin(distances[:, 0]))      # (the first of equal minima: the smaller topic index)
        closest = "the closest pair is topics %d and %d at distance %.17g" % (k, int(ids[k, 0]), float(distances[k, 0]))
    else:
        closest = "there is no pair"
    print("similar topics of snapshot %s: the %d nearest of %d topics by %s distance, %s"
          % (os.path.abspath(snapshot_path), top, len(ids), TOPIC_METRIC, closest))
    with open(similar_path, "w") as output:
        for row_ids, row_distances in zip(ids, distances):
            output.write("\t".join("%d:%.17g" % (k, x) for k, x in zip(row_ids, row_distances)) + "\n")


def report_topic_match(engine, snapshot_path, other_path, match_path):
    """The topics of the snapshot matched one to one with those of the snapshot at other_path: one line on stdout, a line per
    topic in match_path.  TOPIC_MATCH_MISSING / a (TOPIC_MATCH_VOCABULARY, text) pair where it cannot be done, else None."""
    from pylda_amd import topics
    if not os.path.exists(other_path):
        return TOPIC_MATCH_MISSING
    with open(other_path, "rb") as stream:
        other = pickle.load(stream)
    differs = topics.first_differing_word(engine._type_to_index, other._type_to_index)
    if differs:
        return (TOPIC_MATCH_VOCABULARY, differs)
    result = engine.topic_distances(other, TOPIC_METRIC)
    pairs, distances = result.matching()
    print("topic match of snapshot %s with %s: %d of %d topics matched with %d, %s distance mean %g, median %g, maximum %g"
          % (os.path.abspath(snapshot_path), os.path.abspath(other_path), len(pairs), result.values.shape[0], result.values.shape[1],
             TOPIC_METRIC, float(numpy.mean(distances)), float(numpy.median(distances)), float(numpy.max(distances))))
    mine, theirs = engine.top_words(5), other.top_words(5)
    matched = {int(k): (int(other_k), float(x)) for (k, other_k), x in zip(pairs, distances)}
    with open(match_path, "w") as output:
        for k in range(result.values.shape[0]):
            other_k, x = matched.get(k, (-1, numpy.nan))
            output.write("%d\t%d\t%.17g\t%s\t%s\n" % (k, other_k, x, " ".join(str(word) for word, _ in mine[k]),
                                                       " ".join(str(word) for word, _ in theirs[other_k]) if other_k >= 0 else ""))
    return None


def report_topic_coherence(engine, snapshot_path, test_documents, coherence_path, top_words):
    """The engine's topic_coherence() against the test documents: one line on stdout, a line per topic in coherence_path."""
    result = engine.topic_coherence(test_documents, top_words)
    print("topic coherence of snapshot %s over its top %d words on %d documents: UMass %g, NPMI %g (means over %d topics, "
          "%d undefined pairs)" % (os.path.abspath(snapshot_path), result.top_words_count, result.documents, result.umass_mean,
                                   result.npmi_mean, len(result.umass), int(result.undefined_pairs.sum())))
    names = engine._index_to_type
    with open(coherence_path, "w") as output:
        for topic_index in range(len(result.umass)):
            output.write("%d\t%g\t%g\t%s\n" % (topic_index, result.umass[topic_index], result.npmi[topic_index],
                                               "\t".join(str(names.get(int(v), int(v))) for v in result.top_ids[topic_index])))


def evaluate_snapshot(snapshot_path, test_documents, gamma_path, fold_in_samples=-1, fold_in_burn_in=-1, document_completion=0,
                      topic_coherence=0, similar_documents=0, left_to_right=0, left_to_right_resample=1, similar_topics=0,
                      topic_match=None):
    """fold_in_samples >= 0: the engine's fold_in() in place of inference(); None when the engine has none.
    document_completion: the engine's document_completion() in place of either; an engine that folds in still needs
    fold_in_samples (NEEDS_FOLD_IN_SAMPLES without).
    topic_coherence = M > 0: first the coherence of the topics' top M words over the test documents, into coherence-N
    beside gamma_path.
    similar_documents = N > 0: after the test gamma, the N nearest training documents of every test document, into
    similar-N beside gamma_path (NO_TRAINING_ROWS where the snapshot holds no rows of its training documents).
    left_to_right = R > 0: the engine's left_to_right() with R particles in place of all of these (after the coherence):
    one line, no gamma file.
    similar_topics = N > 0: where the coherence runs, the N nearest other topics of every topic, into similar-topics-N.
    topic_match = DIR: there too, the topics matched with those of DIR's snapshot of the same index, into match-N
    (TOPIC_MATCH_MISSING, or (TOPIC_MATCH_VOCABULARY, the difference), where that cannot be done)."""
    with open(snapshot_path, "rb") as stream:
        engine = pickle.load(stream)
    index = os.path.basename(snapshot_path).split("-")[-1]

    def similar(gamma, answer):
        if similar_documents and not report_similar_documents(
                engine, snapshot_path, gamma, os.path.join(os.path.dirname(gamma_path), "similar-" + os.path.basename(snapshot_path).split("-")[-1]),
                similar_documents):
            return NO_TRAINING_ROWS
        return answer
    if topic_coherence:
        report_topic_coherence(engine, snapshot_path, test_documents,
                               os.path.join(os.path.dirname(gamma_path), "coherence-" + os.path.basename(snapshot_path).split("-")[-1]),
                               topic_coherence)
    if similar_topics:
        report_similar_topics(engine, snapshot_path, os.path.join(os.path.dirname(gamma_path), "similar-topics-" + index), similar_topics)
    if topic_match is not None:
        refused = report_topic_match(engine, snapshot_path, os.path.join(topic_match, "model-" + index),
                                     os.path.join(os.path.dirname(gamma_path), "match-" + index))
        if refused is not None:
            return refused
    if left_to_right:
        log_likelihood, tokens, _ = engine.left_to_right(test_documents, left_to_right, bool(left_to_right_resample))
        print("left-to-right likelihood of snapshot %s is %g over %d tokens (per-word perplexity %g)"
              % (os.path.abspath(snapshot_path), log_likelihood, tokens, numpy.exp(-log_likelihood / tokens) if tokens else numpy.nan))
        return log_likelihood
    if document_completion:
        if fold_in_samples >= 0 and not hasattr(engine, "fold_in"):
            return None
        if hasattr(engine, "fold_in"):
            if fold_in_samples < 0:
                return NEEDS_FOLD_IN_SAMPLES
            log_likelihood, tokens, gamma = engine.document_completion(
                test_documents, fold_in_samples, fold_in_burn_in if fold_in_burn_in >= 0 else fold_in_samples // 2)
        else:
            log_likelihood, tokens, gamma = engine.document_completion(test_documents)
        print("document-completion likelihood of snapshot %s is %g over %d held tokens (per-word perplexity %g)"
              % (os.path.abspath(snapshot_path), log_likelihood, tokens, numpy.exp(-log_likelihood / tokens) if tokens else numpy.nan))
        numpy.savetxt(gamma_path, gamma)
        return similar(gamma, log_likelihood)
    if fold_in_samples >= 0:
        if not hasattr(engine, "fold_in"):
            return None
        log_likelihood, gamma = engine.fold_in(test_documents, fold_in_samples,
                                               fold_in_burn_in if fold_in_burn_in >= 0 else fold_in_samples // 2)
    else:
        log_likelihood, gamma = engine.inference(test_documents)
    print("held-out likelihood of snapshot %s is %g" % (os.path.abspath(snapshot_path), log_likelihood))
    numpy.savetxt(gamma_path, gamma)
    return similar(gamma, log_likelihood)


def test_main(argv=None):
    opt = _parse(TEST_FLAGS, argv, "launch_test")
    if opt.input_directory is None or opt.model_directory is None:
        raise SystemExit("--input_directory and --model_directory are required")
    if opt.similar_documents < 0 or opt.similar_documents > 64:
        raise SystemExit("--similar_documents=%d: 0 (off), or 1 .. 64" % opt.similar_documents)
    if opt.left_to_right < 0 or opt.left_to_right > 256 or opt.left_to_right_resample not in (0, 1):
        raise SystemExit("--left_to_right=%d --left_to_right_resample=%d: 0 (off) or 1 .. 256 particles, resample 0 or 1"
                         % (opt.left_to_right, opt.left_to_right_resample))
    if opt.left_to_right and (opt.similar_documents or opt.document_completion):
        raise SystemExit("--left_to_right fits no theta: run it without --similar_documents and --document_completion")
    if opt.similar_topics < 0 or opt.similar_topics > 64:
        raise SystemExit("--similar_topics=%d: 0 (off), or 1 .. 64" % opt.similar_topics)
    source = opt.input_directory.rstrip("/")
    models = opt.model_directory.rstrip("/")
    if opt.topic_match is not None:
        other = opt.topic_match.rstrip("/")
        if not os.path.isdir(other):
            sys.stderr.write("error: --topic_match: model directory %s does not exist...\n" % os.path.abspath(other))
            return 2
        if os.path.basename(os.path.dirname(os.path.abspath(other))) != os.path.basename(source):
            sys.stderr.write("error: --topic_match: corpus name does not match for input (%s) and the models to match (%s)...\n"
                             % (os.path.basename(source), os.path.basename(os.path.dirname(os.path.abspath(other)))))
            return 2
    if not os.path.exists(models):
        sys.stderr.write("error: model directory %s does not exist...\n" % os.path.abspath(models))
        return 1
    trained_on = os.path.basename(os.path.dirname(os.path.abspath(models)))
    if os.path.basename(source) != trained_on:
        sys.stderr.write("error: corpus name does not match for input (%s) and model (%s)...\n"
                         % (os.path.basename(source), trained_on))
        return 1
    _banner((("model_directory", models), ("input_directory", source),
             ("corpus_name", os.path.basename(source)), ("snapshot_index", opt.snapshot_index)))
    held_out = _lines(os.path.join(source, "test.dat"))
    print("successfully load all testing docs from %s..." % os.path.abspath(os.path.join(source, "test.dat")))
    if opt.snapshot_index >= 0:
        wanted = ["model-%d" % opt.snapshot_index]
        if not os.path.exists(os.path.join(models, wanted[0])):
            sys.stderr.write("error: model snapshot %s does not exist...\n"
                             % os.path.abspath(os.path.join(models, wanted[0])))
            return 1
    else:
        wanted = sorted(name for name in os.listdir(models) if name.startswith("model-"))
    for name in wanted:
        answer = evaluate_snapshot(os.path.join(models, name), held_out, os.path.join(models, "test-" + name.split("-")[-1]),
                                   opt.fold_in_samples, opt.fold_in_burn_in, opt.document_completion, opt.topic_coherence,
                                   opt.similar_documents, opt.left_to_right, opt.left_to_right_resample, opt.similar_topics,
                                   opt.topic_match)
        if answer is TOPIC_MATCH_MISSING:
            sys.stderr.write("error: --topic_match: %s holds no snapshot %s to match %s with...\n"
                             % (os.path.abspath(opt.topic_match), name, os.path.abspath(os.path.join(models, name))))
            return 2
        if isinstance(answer, tuple) and answer[0] is TOPIC_MATCH_VOCABULARY:
            sys.stderr.write("error: --topic_match: snapshot %s of %s was trained over another vocabulary: %s...\n"
                             % (name, os.path.abspath(opt.topic_match), answer[1]))
            return 2
        if answer is NEEDS_FOLD_IN_SAMPLES:
            sys.stderr.write("error: --document_completion=1 on snapshot %s, a collapsed Gibbs (mode 1) model: theta is fitted by "
                             "fold-in, give its sweeps with --fold_in_samples...\n" % os.path.abspath(os.path.join(models, name)))
            return 2
        if answer is NO_TRAINING_ROWS:
            sys.stderr.write("error: --similar_documents was given, but snapshot %s holds no rows of its training documents "
                             "(no gamma, no counts) to compare the test documents with...\n" % os.path.abspath(os.path.join(models, name)))
            return 2
        if answer is None:
            sys.stderr.write("error: --fold_in_samples was given, but the engine of snapshot %s has no fold_in (it answers "
                             "inference(): run without the flag)...\n" % os.path.abspath(os.path.join(models, name)))
            return 2
    return 0
