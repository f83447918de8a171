"""The BGZF edge inputs (tests/bgzf_inputs.py) on the CPU: the restatement's block of every case
inflates back to the input with zlib (CRC32, ISIZE, BSIZE), bgzf_block_stats gives bgzf_block's
bytes, and the block's counters reach what the case's builder promises -- so an input holds its
edge independently of the kernel, which tests/test_gpu_bgzf_edges.py runs on the same inputs."""
import numpy as np
import pytest

import bgzf_inputs as B
from oracle import oracle
from test_bgzf import _check_block

RETRIES_MAYBE = ("retries_dist", "retries_codelen")  # the sweep need not reach these (the edge cases do)


def test_edge_cases_hold_their_edges():
    cases = B.edge_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.data) == B.BLOCK, c.name
        blk, st = oracle.bgzf_block_stats(c.data)
        assert blk == oracle.bgzf_block(c.data), c.name
        _check_block(blk, c.data)
        assert st["literals"] + st["matches"] > 0 and st["hlit"] >= 257 and 4 <= st["hclen"] <= 19, c.name
        B.check_want(c, st)


def test_every_retry_path_has_a_case():
    got = {k: 0 for k in ("retries_litlen", "retries_dist", "retries_codelen")}
    for c in B.edge_cases()[:5]:
        st = oracle.bgzf_block_stats(c.data)[1]
        for k in got:
            got[k] += st[k]
    assert all(v >= 1 for v in got.values()), got


def test_retry_searches_give_the_committed_seeds():
    stats_of = lambda d: oracle.bgzf_block_stats(d)[1]
    assert B.search_dist_retry(stats_of, range(8)) == B.DIST_RETRY_SEED
    assert B.search_codelen_retry(stats_of, range(8)) == B.CODELEN_RETRY_SEED


def test_colliding_pairs_collide():
    rng = np.random.default_rng(1)
    for _ in range(8):
        v, u = B.colliding_pair(rng)
        assert v != u and int(B.hash4(v)) == int(B.hash4(u))
        assert int(B.hash4(v)) == ((v * 2654435761) & 0xFFFFFFFF) >> 21


@pytest.mark.parametrize("n", B.SIZES)
def test_sizes(n):
    data = B.sized(n)
    assert len(data) == n
    for o in range(0, n, B.BLOCK):
        chunk = data[o:o + B.BLOCK]
        blk, st = oracle.bgzf_block_stats(chunk)
        _check_block(blk, chunk)
        assert st["literals"] >= 1
        if len(chunk) >= 254:
            assert st["matches"] >= 1


def test_sweep_reaches_every_counter():
    blocks = B.sweep()
    assert len(blocks) == B.SWEEP_BLOCKS and len(set(blocks)) == B.SWEEP_BLOCKS
    top = {k: 0 for k in oracle.BGZF_STATS}
    no_dist = 0
    for d in blocks:
        assert len(d) == B.BLOCK
        blk, st = oracle.bgzf_block_stats(d)
        if blk:
            _check_block(blk, d)
        no_dist += st["dist_used"] == 0
        for k, v in st.items():
            top[k] = max(top[k], v)
    missing = [k for k, v in top.items() if v == 0 and k not in RETRIES_MAYBE]
    assert not missing, missing
    assert no_dist >= 1  # and the other side of dist_used: a block without a match
    assert top["max_dist"] == 32768 and top["max_len"] == 255 and top["hlit"] == 285 and top["hdist"] == 30


def test_many_blocks_contents():
    cs = B.many_contents()
    assert len(set(cs)) == 4
    sizes = {len(oracle.bgzf_block(c)) for c in cs}
    assert len(sizes) == 4 and 0 not in sizes  # different sizes: a wrong prefix sum shows
