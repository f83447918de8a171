"""The GPU BGZF encoder (csrc/bsdc_bgzf.hip) on the inputs of tests/bgzf_inputs.py, whose CPU side
tests/test_bgzf_inputs.py checks: the three Huffman length-limit retries, matches at distance
32767 / 32768 / 32769 and 1 .. 5, match lengths around kLazy, kNice and the segment end, in-round
candidates at the wave boundaries, chains cut at kChain, hash collisions, one- and two-value
blocks, a block without a match; a seeded LZ-style sweep; partial blocks straight through the
C-ABI; and the pack kernel's prefix sum over more than 256 blocks.

Every block: header + deflate bytes equal the restatement's (oracle/bgzf_ref.c), the trailer is 8
zero bytes, and the kernel's own bytes with the host's CRC32 / ISIZE inflate back to the input
with zlib, independently of the restatement.  Byte equality throughout: no tolerance."""
import struct
import zlib

import numpy as np
import pytest

import bgzf_inputs as B
from bsseqconsensusreads_amd import bam
from oracle import oracle
from test_bgzf import _check_block

pytestmark = pytest.mark.gpu

_cache = {}


def ref_block(data: bytes) -> bytes:
    """the restatement's block of `data`, computed once per session."""
    if data not in _cache:
        _cache[data] = oracle.bgzf_block(data)
    return _cache[data]


def inputs(kind):
    if kind not in _cache:
        _cache[kind] = {"edge": lambda: [c.data for c in B.edge_cases()], "sweep": B.sweep,
                        "many": B.many_contents}[kind]()
    return _cache[kind]


def compare(packed: bytes, sizes, blocks, inflate=True):
    """the packed stream against the blocks' restatement bytes; a block that does not fit (no
    input here is known to give one) has size 0 on both sides and no bytes in the stream."""
    assert len(sizes) == len(blocks)
    o = 0
    for k, (s, d) in enumerate(zip(sizes, blocks)):
        ref = ref_block(d)
        assert int(s) == len(ref), (k, int(s), len(ref))
        if not ref:
            continue
        g = packed[o:o + len(ref)]
        o += len(ref)
        assert g[:-8] == ref[:-8], k
        assert g[-8:] == b"\0" * 8, k
        if inflate:
            _check_block(g[:-8] + struct.pack("<II", zlib.crc32(d), len(d)), d)
    assert o == len(packed)


def gpu_compress(g, blocks):
    buf = np.frombuffer(b"".join(blocks), np.uint8).copy()
    packed, sizes = g.compress(buf.ctypes.data, buf.size)
    return packed.tobytes(), sizes


def test_edge_cases_in_one_launch():
    blocks = inputs("edge")
    packed, sizes = gpu_compress(bam.GpuBgzf(0), blocks)
    compare(packed, sizes, blocks)


def test_sweep_in_one_launch():
    blocks = inputs("sweep")
    packed, sizes = gpu_compress(bam.GpuBgzf(0), blocks)
    compare(packed, sizes, blocks)


def test_same_bytes_twice_on_one_encoder():
    """the second job reuses the scratch: re-zeroed slots under the atomicOr, stale tokens, chains
    and distances of the first job's other blocks (the order is rotated)."""
    blocks = inputs("edge")
    g = bam.GpuBgzf(0)
    first, s1 = gpu_compress(g, blocks)
    rot = blocks[7:] + blocks[:7]
    mid, s2 = gpu_compress(g, rot)
    again, s3 = gpu_compress(g, blocks)
    assert first == again and np.array_equal(s1, s3)
    compare(mid, s2, rot, inflate=False)


# ---- partial blocks through the C-ABI ----------------------------------------------------------
def abi_compress(data: bytes):
    """bsdc_bgzf_scratch_bytes / _deflate / _pack on torch device tensors and a torch stream, as
    include/bsdc.h documents them (GpuBgzf only ever sends whole blocks) -> (out bytes with their
    0xEE fill, sizes, the status of a deflate call with blk0 past the input)."""
    import torch

    from bsseqconsensusreads_amd import _lib
    lib = _lib.load()
    n = len(data)
    nblk = -(-n // B.BLOCK)
    dev = torch.device("cuda:0")
    din = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    scratch = torch.empty(int(lib.bsdc_bgzf_scratch_bytes(nblk)), dtype=torch.uint8, device=dev)
    sizes = torch.full((nblk,), -7, dtype=torch.int32, device=dev)
    out = torch.full((nblk * 65536,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        past = lib.bsdc_bgzf_deflate(din.data_ptr(), n, nblk, 1, scratch.data_ptr(), sizes.data_ptr(), st)
        stream.synchronize()
        assert (sizes == -7).all()  # nothing ran
        assert lib.bsdc_bgzf_deflate(din.data_ptr(), n, 0, nblk, scratch.data_ptr(), sizes.data_ptr(), st) == 0
        assert lib.bsdc_bgzf_pack(scratch.data_ptr(), sizes.data_ptr(), 0, nblk, out.data_ptr(), st) == 0
    stream.synchronize()
    return out.cpu().numpy().tobytes(), sizes.cpu().numpy(), past


@pytest.mark.parametrize("n", B.SIZES)
def test_sizes_through_the_abi(n):
    data = B.sized(n)
    out, sizes, past = abi_compress(data)
    assert past == -22
    blocks = [data[o:o + B.BLOCK] for o in range(0, n, B.BLOCK)]
    assert len(blocks) == (2 if n > B.BLOCK else 1) and len(blocks[-1]) == (n - 1) % B.BLOCK + 1
    total = int(sizes.sum())
    compare(out[:total], sizes, blocks)  # back to back from byte 0
    assert out[total:] == b"\xee" * (len(out) - total)  # and nothing behind them


# ---- the pack kernel over more than 256 blocks ---------------------------------------------------
@pytest.mark.parametrize("max_blocks", [None, 100])
def test_pack_over_260_blocks(monkeypatch, max_blocks):
    """260 blocks cycled from 4 contents of different compressed sizes: one launch (the prefix sum
    of block 259 takes a second trip of the 256-thread loop), and launches of 100 (blk0 = 100, 200:
    the earlier launches' sizes summed on the device)."""
    if max_blocks:
        monkeypatch.setattr(bam.GpuBgzf, "MAX_BLOCKS", max_blocks)
    cs = inputs("many")
    blocks = [cs[k % 4] for k in range(B.MANY_BLOCKS)]
    packed, sizes = gpu_compress(bam.GpuBgzf(0), blocks)
    assert len(packed) == sum(len(ref_block(c)) for c in blocks) == int(sizes.sum())
    compare(packed, sizes, blocks, inflate=False)
    compare(packed[:sum(len(ref_block(c)) for c in cs)], sizes[:4], cs)  # the 4 contents inflate
