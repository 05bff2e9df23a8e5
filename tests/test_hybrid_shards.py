"""launch_train --gpus N with the hybrid engine, start-up on CPU (gloo): every rank's Hybrid learns the global index
of its first document, so that the sampler's counter-based streams name the documents as a one-process run does."""
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _documents():
    rng = np.random.default_rng(11)
    return [" ".join("w%d" % t for t in rng.integers(0, 34, rng.integers(0, 25))) for _ in range(53)]   # (some empty)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from pylda_amd import cli
    from pylda_amd.hybrid import Hybrid
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    engine = Hybrid(device=0, process_group=None, seed=5)
    engine._verbose = False
    cli._initialize_shard(engine, _documents(), ["w%d" % i for i in range(30)], 4, 0.25, 1.0 / 30, rank, world)
    np.savez(os.path.join(out_dir, "shard%d.npz" % rank), D=engine._number_of_documents, first=engine._first_document,
             ptr=engine._train_csr[0])
    dist.destroy_process_group()


def test_each_rank_knows_its_first_global_document(tmp_path):
    import torch.multiprocessing as mp
    world = 3
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    shards = [np.load(tmp_path / ("shard%d.npz" % r)) for r in range(world)]
    sys.path.insert(0, ROOT)
    from pylda_amd import _capi
    ptr, _, _, _ = _capi.parse_corpus(_documents(), ["w%d" % i for i in range(30)])
    assert sum(int(s["D"]) for s in shards) == len(ptr) - 1
    assert [int(s["first"]) for s in shards] == [0, int(shards[0]["D"]), int(shards[0]["D"]) + int(shards[1]["D"])]
    assert all(int(s["D"]) > 0 for s in shards)
