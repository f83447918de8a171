"""The BGZF inflate's host twin (bsdc_bgzf_inflate_host, csrc/bsdc_inflate.hip) on the edge lists of
tests/inflate_inputs.py -- copies(), rounds(), tables(), placements() and flips() -- against zlib:
valid blocks byte for byte, the guard bytes intact, every single-bit flip accepted or refused as
zlib does.  Then the same blocks through tests/sanitize/inflate_twin_main.cpp, a stand-alone
program built with ASan and UBSan that holds `comp` and `out` in heap buffers of their exact
sizes, against the in-process twin.  No GPU: tests/test_gpu_inflate_edges.py runs on one only
streams that went through here first."""
import dataclasses
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from bsseqconsensusreads_amd import _lib as L

import inflate_inputs as I
from test_inflate_host import GUARD, check, host_inflate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 4  # bytes of 0xFF before every block in `comp`, at least: bits a reader past clen would not take for zeros


def layout_at(placed):
    """(comp bytes, block table, out size) of (block, src % 4, dst % 16) triples: every block's
    compressed bytes and window at the residues asked for, PAD.. bytes of 0xFF between the
    compressed blocks, GUARD.. bytes between the windows."""
    comp = bytearray()
    d = (L.InflateBlockC * len(placed))()
    dst = 0
    for i, (b, sm, dm) in enumerate(placed):
        comp += b"\xff" * PAD
        comp += b"\xff" * ((sm - len(comp)) % 4)
        dst += GUARD
        dst += (dm - dst) % 16
        d[i].src, d[i].clen, d[i].isize, d[i].dst = len(comp), len(b.comp), b.isize, dst
        assert d[i].src % 4 == sm and d[i].dst % 16 == dm
        comp += b.comp
        dst += b.isize
    return bytes(comp), d, dst + GUARD


def spread(blocks):
    """a list without placements of its own: the residues in turn"""
    return [(b, i % 4, (5 * i) % 16) for i, b in enumerate(blocks)]


def host_inflate_at(placed):
    comp, d, n_out = layout_at(placed)
    ca = np.frombuffer(comp + b"\0", np.uint8)
    out = np.full(n_out, 0xA5, np.uint8)
    status = np.full(len(placed), -1, np.int32)
    assert L.load().bsdc_bgzf_inflate_host(ca.ctypes.data, len(comp), d, len(placed), out.ctypes.data, n_out,
                                           status.ctypes.data) == 0
    return d, out, status


def check_flips(blocks, d, out, status, twin_status=None):
    """check() where a refused flip (code ANY) may have any nonzero status"""
    for i, b in enumerate(blocks):
        if b.code == I.ANY:
            assert b.want is None and status[i] != 0, (b.name, "zlib refuses it")
    check([dataclasses.replace(b, code=int(status[i])) if b.code == I.ANY else b for i, b in enumerate(blocks)],
          d, out, status, twin_status)


@pytest.mark.parametrize("name", ["copies", "rounds", "tables"])
def test_edge_lists_equal_zlib(name):
    blocks = getattr(I, name)()
    assert sum(b.want is not None for b in blocks) >= 13
    check(blocks, *host_inflate(blocks))
    check(blocks, *host_inflate_at(spread(blocks)))


def test_rejected_table_fixtures_are_rejected_by_zlib_too():
    bad = [b for b in I.tables() if b.want is None]
    assert sorted(b.name for b in bad) == ["hclen_4_has_no_end_of_block", "run_18_of_138_across_hlit_hdist",
                                           "stale_unused_distance_code"]
    for b in bad:
        with pytest.raises(zlib.error):
            I.ref(b.comp)


def test_placements_equal_zlib():
    placed = I.placements()
    for n in I.DST_ISIZES:
        assert {dm for b, _, dm in placed if b.name.startswith("isize_%d_dst" % n)} == set(range(16))
    for name in ["clen_%d" % n for n in I.SRC_CLENS] + ["clen_5_stored_empty", "costliest_round", "largest_header"]:
        got = [(len(b.comp), sm) for b, sm, _ in placed if b.name.startswith(name + "_src")]
        assert [sm for _, sm in got] == [0, 1, 2, 3], name
    blocks = [b for b, _, _ in placed]
    assert [b.name for b in blocks if b.want is None] == ["clen_1_src_%d" % s for s in range(4)]
    for b in blocks:
        if b.want is None:  # the one shape with no valid block: zlib refuses it too
            with pytest.raises(zlib.error):
                I.ref(b.comp)
    check(blocks, *host_inflate_at(placed))


def test_every_single_bit_flip_follows_zlib():
    blocks = I.flips()
    assert len(blocks) == sum(8 * len(c) for _, c in I.flip_bases()) > 8 * (105 + 16)  # none left out
    for name, _ in I.flip_bases():
        mine = [b for b in blocks if b.name.startswith(name + "_bit_")]
        assert any(b.want is None for b in mine) and any(b.want is not None for b in mine)
    check_flips(blocks, *host_inflate(blocks))


def everything():
    """all lists in one layout, the earlier ones of tests/test_inflate_host.py too"""
    blocks = I.valid() + I.corrupt() + I.copies() + I.rounds() + I.tables() + I.flips()
    return spread(blocks) + list(I.placements())


@pytest.fixture(scope="module")
def twin_program(tmp_path_factory):
    """tests/sanitize/inflate_twin_main.cpp + csrc/bsdc_inflate.hip, the host side under ASan and UBSan"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed (the build needs it too)"
    exe = str(tmp_path_factory.mktemp("twin") / "inflate_twin_asan")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "inflate_twin_main.cpp"),
           os.path.join(ROOT, "bsseqconsensusreads_amd", "csrc", "bsdc_inflate.hip"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def test_sanitized_twin_on_exact_buffers_equals_the_twin(twin_program, tmp_path):
    placed = everything()
    comp, d, n_out = layout_at(placed)
    src, dst = str(tmp_path / "blocks.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qqq", len(placed), len(comp), n_out))
        f.write(bytes(d))
        f.write(comp)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (leaks: the HIP runtime it links, not the code under test)
    p = subprocess.run([twin_program, src, dst], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "inflate_twin ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-4000:])
    raw = open(dst, "rb").read()
    status = np.frombuffer(raw[:4 * len(placed)], np.int32)
    out = np.frombuffer(raw[4 * len(placed):], np.uint8)
    assert out.shape[0] == n_out
    _, twin_out, twin_status = host_inflate_at(placed)
    assert np.array_equal(status, twin_status) and np.array_equal(out, twin_out)
    check_flips([b for b, _, _ in placed], d, out, status)
