"""The BGZF inflate kernel (k_inflate, csrc/bsdc_inflate.hip) on the edge lists of
tests/inflate_inputs.py, where the wave runs what the host twin runs on one lane or not at all:
copy_match over 64 lanes (copies), the 256-token ring and the 2 KiB compressed window (rounds),
huff_build across lanes (tables), the write-out and the window's first dword at every alignment
(placements), and every single-bit flip of four small streams (flips).  One launch per list,
against zlib's bytes, status 0 for every valid block, every byte outside the windows still 0xA5.

Order: tests/test_inflate_edges.py runs the same streams, the flipped ones included, through the
host twin and through the sanitizer program on the CPU; this file only imports those streams.
Run the two in one command, the CPU file first:
    pytest tests/test_inflate_edges.py tests/test_gpu_inflate_edges.py"""
import pytest

import inflate_inputs as I
from test_gpu_inflate import Device
from test_inflate_edges import check_flips, host_inflate_at, layout_at, spread
from test_inflate_host import check

pytestmark = pytest.mark.gpu


def run_at(placed):
    blocks = [b for b, _, _ in placed]
    return blocks, Device(blocks, layout_at(placed)).run()


@pytest.mark.parametrize("name", ["copies", "rounds", "tables"])
def test_edge_list_equals_zlib(engine, name):
    blocks, got = run_at(spread(getattr(I, name)()))
    check(blocks, *got)
    assert all(got[2][i] == 0 for i, b in enumerate(blocks) if b.want is not None)


def test_placements_equal_zlib(engine):
    blocks, got = run_at(I.placements())
    check(blocks, *got)


def test_every_single_bit_flip_gets_the_twins_status(engine):
    """all flips of all four base streams in one launch: the twin's status value for value, zlib's
    bytes for the flips zlib accepts, the guards intact.  Every stream here has gone through the
    twin and the sanitizer program on the CPU first (tests/test_inflate_edges.py; see above)."""
    placed = spread(I.flips())
    _, _, twin = host_inflate_at(placed)
    blocks, got = run_at(placed)
    assert len(blocks) == sum(8 * len(c) for _, c in I.flip_bases())  # none left out
    check_flips(blocks, *got, twin_status=twin)
