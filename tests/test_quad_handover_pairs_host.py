"""The hand-over tile in slot pairs (estep_quad.h quad_hand_over, estep_limits.h quad_handover_pairs): which bytes of a
column every thread of a stride-256 document stores, from the index function the kernel itself uses (quad_pair_store),
compiled for the host by tests/native/quad_pairs_table.cpp.  No GPU.

For every N = 1 .. 256 and every stride-256 geometry the planner emits (10 register slots with 0 .. 4 LDS slots, 8 with
none, 8 + 4 with 1 .. 4 streamed slots):
  - the byte ranges stored into a column, over all 512 threads and all store indices, cover [0, 8 N) exactly once (the
    terms a geometry has slots for: 16 per slot), and nothing lies at or beyond 8 N - a 16-byte store past N would land in
    the next column and, in a document's last column, beyond its region of the buffer;
  - every 16-byte store starts at an even term, every 8-byte store of a pair at the last term of an odd-length document;
  - the terms are the ones the two word groups of a wavefront hold in the slot (a restatement in Python of the layout:
    term 16 s + 2 wave + {0, 1}), the lower half-wave storing slot 2 q and the upper one slot 2 q + 1."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (on-chip slots, all slots)
GEOMETRIES = [(8, 8)] + [(10 + twl, 10 + twl) for twl in range(5)] + [(12, 12 + swl) for swl in range(1, 5)]


@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    cxx = next((c for c in (shutil.which(n) for n in ("g++", "c++", "clang++")) if c), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("quad_pairs") / "quad_pairs_table")
    build = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "quad_pairs_table.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.mark.parametrize("wpr,wpg", GEOMETRIES)
def test_paired_stores_cover_every_column_exactly_once(table_program, wpr, wpg):
    pairs, stores = (wpr + 1) // 2, (wpr + 1) // 2 + wpg - wpr
    raw = subprocess.run([table_program, str(wpr), str(wpg)], capture_output=True, check=True).stdout
    table = np.frombuffer(raw, np.int16).reshape(256, 512, stores, 2).astype(np.int64)
    term, nbytes = table[..., 0], table[..., 1]
    N, tid, q = np.broadcast_arrays(np.arange(1, 257)[:, None, None], np.arange(512)[None, :, None], np.arange(stores)[None, None, :])
    wave, upper = tid // 64, tid // 32 % 2
    assert set(np.unique(nbytes)) <= {0, 8, 16}
    assert np.all(nbytes[:, :, pairs:] <= 8)                       # streamed slots: one term per lane
    stored = nbytes > 0
    # nothing at or beyond 8 N
    assert np.all((term * 8 + nbytes <= 8 * N)[stored])
    assert np.all(term[stored] >= 0)
    # 16 bytes: from an even term; 8 bytes of a pair: the last term of an odd length
    assert np.all(term[nbytes == 16] % 2 == 0)
    single = (nbytes == 8) & (q < pairs)
    assert np.all((term == N - 1)[single]) and np.all((N % 2 == 1)[single])
    # the layout restated: on-chip slot s = 2 q + upper of word groups 2 wave and 2 wave + 1; streamed slot s of word
    # group 2 wave + upper, groups in reverse order
    on_chip = stored & (q < pairs)
    s = 2 * q + upper
    assert np.all((term == 16 * s + 2 * wave)[on_chip]) and np.all((s < wpr)[on_chip])
    streamed = stored & (q >= pairs)
    s = wpr + q - pairs
    assert np.all((term == 16 * s + 15 - (2 * wave + upper))[streamed])
    # a column belongs to one topic, held by ONE of the 32 topic lanes (tid % 32) of every half-wave - and what a lane
    # stores does not depend on which: every term the geometry has a slot for, exactly once per column
    by_lane = table.reshape(256, 16, 32, stores, 2)
    assert np.array_equal(by_lane, np.broadcast_to(by_lane[:, :, :1], by_lane.shape))
    count = np.zeros((256, 258), np.int64)
    one, both = stored & (tid % 32 == 0), (nbytes == 16) & (tid % 32 == 0)
    np.add.at(count, (N[one] - 1, term[one]), 1)
    np.add.at(count, (N[both] - 1, term[both] + 1), 1)
    for n_terms in range(1, 257):
        held = min(n_terms, 16 * wpg)
        assert np.all(count[n_terms - 1, :held] == 1), (n_terms, count[n_terms - 1, :held])
        assert np.all(count[n_terms - 1, held:] == 0), n_terms
