"""The pure-Python restatement of cli zipper's rules (tests/zipper_ref.py) against hand-written
answers, and the edge inputs (tests/zipper_inputs.py) against the edges they are named for."""
import struct

import pytest

import zipper_inputs as ZI
import zipper_ref as ZR

T, rec = ZI.tag, ZI.rec


def _zip(a, u, **kw):
    out, counts = ZR.zip_records(ZR.parse_records(b"".join(a)), ZR.parse_records(b"".join(u)), **kw)
    return out, counts


def test_override_and_removal():
    a = [rec("r", 99, 0, 5, aux=T("NM", "i", 2) + T("RG", "Z", "bwa") + T("MD", "Z", "5"))]
    u = [rec("r", 77, aux=T("RG", "Z", "A") + T("MI", "Z", "1/A") + T("XR", "Z", "q"))]
    out, _ = _zip(a, u)
    assert out[0]["aux"] == b"NMi\2\0\0\0MDZ5\0RGZA\0MIZ1/A\0XRZq\0"  # the aligned RG gives way to the partner's
    out, _ = _zip(a, u, remove=["XR", "NM"])
    assert out[0]["aux"] == b"MDZ5\0RGZA\0MIZ1/A\0"
    assert out[0]["flag"] == 99 and out[0]["pos"] == 5 and out[0]["name"] == b"r"


def test_reverse_and_revcomp():
    part = T("cd", "B", ("s", [1, 2, 3])) + T("ac", "Z", "ACGTNacgt-") + T("cD", "i", 7)
    a = [rec("r", 83, 0, 5), rec("r", 163, 0, 6)]
    u = [rec("r", 77, aux=part), rec("r", 141, aux=part)]
    out, _ = _zip(a, u, reverse=["Consensus"], revcomp=["Consensus"])
    assert out[0]["flag"] == 83
    assert out[0]["aux"] == b"cdBs\3\0\0\0\3\0\2\0\1\0" + b"acZ-acgtNACGT\0" + b"cDi\7\0\0\0"
    assert out[1]["flag"] == 163 and out[1]["aux"] == part  # a forward record is left alone
    out, _ = _zip(a, u, reverse=["ac"])  # reversed, not complemented
    assert out[0]["aux"] == part[:14] + b"acZ-tgcaNTGCA\0" + b"cDi\7\0\0\0"
    out, _ = _zip(a, u, revcomp=["cd", "cD"])  # not a Z tag: unchanged
    assert out[0]["aux"] == part
    out, _ = _zip(a, u)
    assert out[0]["aux"] == part


def test_a_payload_that_reads_like_a_tag_stays_whole():
    spell = T("zz", "B", ("C", list(b"MIZx\0XRZ"))) + T("zy", "Z", "NMiXRZ")
    a = [rec("r", 99, 0, 5, aux=spell + T("NM", "i", 1))]
    u = [rec("r", 77, aux=T("MI", "Z", "1"))]
    out, _ = _zip(a, u, remove=["XR"])
    assert out[0]["aux"] == spell + T("NM", "i", 1) + T("MI", "Z", "1")


def test_tie_order_drop_and_counts():
    a = [rec("a", 99, 1, 7), rec("b", 83, 0, 9), rec("c", 99, 0, 9), rec("d", 83, 0, 9), rec("e", 99, 0, 9),
         rec("f", 99, 0, 8), rec("g", 77, 0, 9), rec("b", 147, 0, 0)]
    u = [rec(n, 77) for n in "abcdefg"] + [rec("b", 141), rec("h", 77), rec("h", 141)]
    out, counts = _zip(a, u)
    assert [r["name"] for r in out] == [b"b", b"f", b"c", b"e", b"b", b"d", b"a"]
    assert counts == dict(records_in=8, records_out=7, unmapped_dropped=1, templates_without_aligned=1)


def test_flag_200_is_the_partners():
    out, _ = _zip([rec("r", 99 | 0x200, 0, 1), rec("r", 147, 0, 2)], [rec("r", 77), rec("r", 141 | 0x200)])
    assert [r["flag"] for r in out] == [99, 147 | 0x200]


def test_errors():
    with pytest.raises(ValueError, match="no partner"):
        _zip([rec("r", 99, 0, 1)], [rec("r", 141)])
    with pytest.raises(ValueError, match="twice"):
        _zip([rec("r", 99, 0, 1)], [rec("r", 77), rec("r", 77)])
    with pytest.raises(ValueError, match="unknown type"):
        _zip([rec("r", 99, 0, 1, aux=b"XYq\1")], [rec("r", 77)])
    with pytest.raises(ValueError, match="runs past"):
        _zip([rec("r", 99, 0, 1)], [rec("r", 77, aux=b"cdBs\3\0\0\0\1\0")])


def test_header():
    assert ZR.header_text(ZI.HEADER_A, ZI.HEADER_U) == (
        "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:900000000\n@SQ\tSN:chr2\tLN:5000\n@SQ\tSN:chr3\tLN:5000\n"
        "@RG\tID:A\tSM:s\n@PG\tID:bwameth\tPN:bwameth\n@PG\tID:samtools\tPN:samtools\n@PG\tID:fgbio\tPN:fgbio\n"
        "@CO\taligned\n@CO\tunmapped\n")


def test_encode_round_trip():
    data = b"".join(ZI.case("all")[0])
    assert b"".join(ZR.encode(r) for r in ZR.parse_records(data)) == data


def test_every_edge_input_holds_its_edge():
    P = lambda k: tuple(ZR.parse_records(b"".join(x)) for x in ZI.case(k))  # noqa: E731
    tags = lambda r: {nm: (t, b) for nm, t, b in ZR.walk(r["aux"])}  # noqa: E731
    a, u = P("names")
    assert sorted(len(r["name"]) for r in a) == [1, 254]
    a, u = P("aux_empty")
    by = {(r["name"], r["flag"] & 0xC0): r for r in u}
    kinds = {(bool(r["aux"]), bool(by[(r["name"], r["flag"] & 0xC0)]["aux"])) for r in a}
    assert kinds == {(False, True), (True, False), (False, False)}
    a, u = P("both_sides")
    assert set(tags(a[0])) & set(tags(u[0])) >= {"NM".encode(), b"RG", b"MI"}
    a, u = P("spelled")
    t = tags(a[0])
    assert t[b"zz"][0] == "B" and b"MIZ" in t[b"zz"][1] and b"XRZ" in t[b"zz"][1] and t[b"zy"][0] == "Z" and b"XRZ" in t[b"zy"][1]
    assert b"XR" in ZR.expand(ZI.SETTINGS["remove"]["remove"], [])
    a, u = P("b_subtypes")
    t = tags(u[0])
    assert {chr(b[3]) for _, b in t.values()} == set("cCsSiIf")
    assert {struct.unpack_from("<I", b, 4)[0] for _, b in t.values()} == {0, 1, 2, 5}
    assert all(r["flag"] & 16 for r in a[:1]) and set(t) <= {x.encode() for x in ZR.CONSENSUS_REVERSE}
    a, u = P("z_lens")
    assert {len(b) - 4 for ty, b in tags(u[0]).values() if ty == "Z"} == {0, 1, 2} and a[0]["flag"] & 16
    a, u = P("odd_zero")
    assert a[0]["l_seq"] % 2 == 1 and a[1]["cigar"] == [] and a[2]["l_seq"] == 0
    a, u = P("sec_supp")
    assert [bool(r["flag"] & 0x800) for r in a][0] and any(r["flag"] & 0x100 for r in a) and len({r["name"] for r in a}) == 1
    a, u = P("fragment")
    assert all(r["flag"] & 0xC0 == 0 for r in a + u) and {r["flag"] & 16 for r in a} == {0, 16}
    a, u = P("bit200")
    assert [bool(r["flag"] & 0x200) for r in a] == [False, True] and [bool(r["flag"] & 0x200) for r in u] == [True, False]
    a, u = P("unmapped_mate")
    assert [bool(r["flag"] & 4) for r in a] == [False, True] and {r["name"] for r in u} - {r["name"] for r in a} == {b"lonely", b"lonely2"}
    a, u = P("long")
    assert len(ZR.encode(a[0])) > 65280
    a, u = P("ties")
    assert len({(r["ref"], r["pos"], r["flag"] & 16) for r in a}) < len(a) and {r["pos"] for r in a} >= {0, 1 << 29}
    a, u = P("all")
    assert len(a) == sum(len(ZI.case(k)[0]) for k in ZI.NAMES[:-1])
    assert [(r["ref"], r["pos"]) for r in a] != sorted((r["ref"], r["pos"]) for r in a)
    for k in ZI.ERRORS:
        ea, eu, _ = ZI.error_case(k)
        with pytest.raises(ValueError):
            ZR.zip_records(ZR.parse_records(b"".join(ea)), ZR.parse_records(b"".join(eu)))
    n = {k: len(ZI.sort_case(k)[0]) for k in ZI.SORTS}
    assert (n["n0"], n["n1"], n["n255"], n["n256"], n["n257"], n["tile_plus_1"], n["two_tiles_plus_1"]) == (0, 1, 255, 256, 257, 2049, 4097)
