"""k_filter (csrc/bsdc_filter.hip) on the fabricated rows of tests/filter_rows.py
(whose ground test_filter_rows.py checks on the CPU) against tests/filter_ref.py: filt, masked and
the whole seq / qual buffers byte for byte -- the reference's masked values inside the lengths, the
bytes that went in everywhere else: past the lengths, in ends that failed the gate, in families not
emitted and in 64 guard bytes on either side -- with the ss_* rows unchanged; the rows of
bamrec_inputs.py through the filter too; the kernel's read-rate verdicts against the E tags the host
encoder writes for the same rows; and the launcher's refusals.  Every comparison is exact."""
import ctypes as C
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bamrec_inputs as BI
import filter_inputs as FI
import filter_ref as FR
import filter_rows as W
from bsseqconsensusreads_amd import _lib, bam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Call:
    """bsdc_filter's arguments for a FilterRows, on the device: seq, qual, filt and masked between
    guards of 0xA5, every base 16-byte aligned."""

    def __init__(self, engine, x: W.FilterRows):
        self.engine, self.x, self.F = engine, x, x.n_fam
        pad = lambda a: a if a.size else np.zeros(16, a.dtype)  # noqa: E731
        self.host = {"status": x.status, "len": x.length.astype(np.uint16), "ss_len": x.ss_len.astype(np.uint16),
                     "ss_base": x.ss_base, "ss_qual": x.ss_qual, "ss_depth": x.ss_depth, "ss_err": x.ss_err}
        if x.ss_wide is not None:
            self.host.update(ss_wide=x.ss_wide, ss_wdepth=x.ss_wdepth, ss_werr=x.ss_werr)
        self.host = {k: _bytes(pad(v)) for k, v in self.host.items()}
        self.dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in self.host.items()}
        self.seq0, self.qual0 = self._guarded(_bytes(x.seq)), self._guarded(_bytes(x.qual))
        self.seq, self.qual = torch.from_numpy(self.seq0).to(DEV), torch.from_numpy(self.qual0).to(DEV)
        self.filt = torch.empty(2 * GUARD + self.F, dtype=torch.uint8, device=DEV)
        self.masked = torch.empty(2 * GUARD + 4 * self.F, dtype=torch.uint8, device=DEV)
        o = self.o = _lib.ConsensusC()
        o.stride = x.stride
        o.seq, o.qual = self.seq.data_ptr() + GUARD, self.qual.data_ptr() + GUARD
        for k, t in self.dev.items():
            setattr(o, k, t.data_ptr())
        for t in list(self.dev.values()) + [self.seq, self.qual, self.filt, self.masked]:
            assert t.data_ptr() % 16 == 0

    @staticmethod
    def _guarded(a):
        return np.concatenate([np.full(GUARD, 0xA5, np.uint8), a, np.full(GUARD, 0xA5, np.uint8)])

    def run(self, p: dict, kind=None, n_fam=None, filt=True, **o_fields):
        """one launch under the parameter set p (restoring seq / qual first) -> (rc, the four guarded
        buffers as they came back); o_fields override fields of the bsdc_consensus for this call"""
        self.seq.copy_(torch.from_numpy(self.seq0))
        self.qual.copy_(torch.from_numpy(self.qual0))
        self.filt.fill_(0xA5)
        self.filt[GUARD:GUARD + self.F] = 0xAA
        self.masked.fill_(0xA5)
        self.masked[GUARD:GUARD + 4 * self.F] = 0xFF
        o = _lib.ConsensusC.from_buffer_copy(self.o)
        for k, v in o_fields.items():
            setattr(o, k, v)
        fp = FI.filter_params(p).c_struct()
        rc = self.engine.lib.bsdc_filter(self.engine.ctx, C.byref(fp), self.x.kind if kind is None else kind,
                                         self.F if n_fam is None else n_fam, C.byref(o),
                                         C.c_void_p(self.filt.data_ptr() + GUARD) if filt else None,
                                         C.c_void_p(self.masked.data_ptr() + GUARD),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, {k: getattr(self, k).cpu().numpy() for k in ("seq", "qual", "filt", "masked")}

    def untouched(self):
        """filt / masked as run() fills them before the launch"""
        f, m = np.full(2 * GUARD + self.F, 0xA5, np.uint8), np.full(2 * GUARD + 4 * self.F, 0xA5, np.uint8)
        f[GUARD:GUARD + self.F], m[GUARD:GUARD + 4 * self.F] = 0xAA, 0xFF
        return {"seq": self.seq0, "qual": self.qual0, "filt": f, "masked": m}

    def check(self, p: dict, ref, what):
        """one launch -> the device's filt; everything asserted against the reference `ref`"""
        filt, masked, seq, qual = ref
        rc, got = self.run(p)
        assert rc == 0, (what, self.engine.lib.bsdc_last_error(self.engine.ctx))
        gf = got["filt"][GUARD:GUARD + self.F]
        bad = np.nonzero(gf != filt)[0]
        assert bad.size == 0, "%s: filt differs at families %s: gpu %s ref %s" % (what, bad[:8], gf[bad[:8]], filt[bad[:8]])
        gm = got["masked"][GUARD:GUARD + 4 * self.F].view(np.uint16).astype(np.int32).reshape(self.F, 2)
        bad = np.nonzero((gm != masked).any(axis=1))[0]
        assert bad.size == 0, "%s: masked differs at families %s: gpu %s ref %s" % (what, bad[:8], gm[bad[:8]], masked[bad[:8]])
        for k in ("filt", "masked"):
            assert (got[k][:GUARD] == 0xA5).all() and (got[k][-GUARD:] == 0xA5).all(), (what, k, "guards")
        for k, want in (("seq", W.pack(seq)), ("qual", qual)):
            want = self._guarded(_bytes(want))
            bad = np.nonzero(got[k] != want)[0]
            if bad.size:
                at = int(bad[0]) - GUARD
                per = self.x.stride // (2 if k == "seq" else 1)
                raise AssertionError("%s: %d %s bytes differ, the first in family %d end %d at byte %d: gpu %d ref %d" % (
                    what, bad.size, k, at // (2 * per), at // per % 2, at % per, got[k][bad[0]], want[bad[0]]))
        for k, t in self.dev.items():
            assert np.array_equal(t.cpu().numpy(), self.host[k]), (what, k, "changed")
        return gf


@pytest.mark.parametrize("name", W.SETS)
def test_fabricated_rows_equal_the_reference(engine, name):
    x = W.make(name)
    c = _Call(engine, x)
    for pn, p in x.params.items():
        c.check(p, W.reference(name, pn), "%s / %s" % (name, pn))


@pytest.mark.parametrize("stride", [16, 32, 528])
def test_bamrec_rows_equal_the_reference(engine, stride):
    """the BAM record path's fabricated rows (disagreeing strands, wide rows, garbage, errors above
    depth, every seq code and quality byte) through the filter, both kinds"""
    b = BI.make(stride)
    for kind in (0, 1):
        x = W.FilterRows("bamrec%d" % stride, kind, stride, b.status, b.length, b.seq, b.qual, b.ss_len, b.ss_base, b.ss_qual,
                         b.ss_depth, b.ss_err, b.ss_wide, b.ss_wdepth, b.ss_werr, {})
        c = _Call(engine, x)
        n_dropped = n_masked = 0
        for pn in ("typical", "single_ok", "agree", "fgbio_defaults"):
            ref = x.apply(FI.PARAM_SETS[pn])
            c.check(FI.PARAM_SETS[pn], ref, "bamrec %d / kind %d / %s" % (stride, kind, pn))
            n_dropped += int((ref[0] != 0).sum())
            n_masked += int(ref[1].sum())
        assert n_dropped and n_masked


def _e_tags(aux: bytes) -> dict:
    """the float tags of one record's consensus tags (cE, aE, bE), walking the aux fields"""
    size = {ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
    out, o = {}, 0
    while o < len(aux):
        tag, ty = aux[o:o + 2].decode(), aux[o + 2]
        o += 3
        if ty == ord("Z"):
            o = aux.index(b"\0", o) + 1
        elif ty == ord("B"):
            o += 5 + size[aux[o]] * struct.unpack_from("<i", aux, o + 1)[0]
        else:
            if ty == ord("f"):
                out[tag] = np.frombuffer(aux, "<f4", 1, o)[0]
            o += size[ty]
    return out


@pytest.mark.parametrize("name", ["gate32", "gate32_mol"])
def test_read_rate_verdicts_are_the_tags(engine, name):
    """a tagged BAM and the filter see one rate: READERR on the gate is float(tag) > T under the
    min / max rule, with cE, aE, bE read as float32 from the host encoder's tag bytes"""
    x = W.make(name)
    cons = SimpleNamespace(length=x.length, ss=x.ref_args()[0])
    tab = bam.consensus_tags(cons, np.arange(x.n_fam), bool(x.kind), 2)
    tags = [_e_tags(bytes(tab.buf[tab.off[k]:tab.off[k + 1]])) for k in range(2 * x.n_fam)]
    assert all("cE" in t for t in tags) and (x.kind == 1 or all("aE" in t for t in tags))
    assert x.kind == 1 or any("bE" in t for t in tags) and any("bE" not in t for t in tags)
    nan0 = lambda v: 0.0 if v != v else float(v)  # noqa: E731
    c = _Call(engine, x)
    for pn, p in x.params.items():
        T = FR.three(p["max_read_error_rate"])
        want = np.zeros(x.n_fam, bool)
        for k, t in enumerate(tags):
            drop = float(t["cE"]) > T[0]
            if x.kind == 0:
                a, b = nan0(t["aE"]), nan0(t.get("bE", np.float32(0)))
                drop |= min(a, b) > T[1] or max(a, b) > T[2]
            want[k // 2] |= drop
        rc, got = c.run(p)
        assert rc == 0
        gf = got["filt"][GUARD:GUARD + x.n_fam]
        assert np.array_equal((gf & FR.READERR) != 0, want), pn


def test_refusals_and_a_good_call_after_them(engine):
    x = W.make("reads")
    assert x.ss_wide is not None
    c = _Call(engine, x)
    p = x.params["M2_1_0"]
    o = c.o
    off = lambda k: getattr(o, k) + 8  # noqa: E731
    cases = [("stride", dict(stride=0)), ("stride", dict(stride=8)), ("stride", dict(stride=24)),
             ("aligned", dict(seq=off("seq"))), ("aligned", dict(qual=off("qual"))), ("aligned", dict(ss_depth=off("ss_depth"))),
             ("aligned", dict(ss_wdepth=off("ss_wdepth"))), ("ss_wdepth", dict(ss_wdepth=None)), ("null", dict(filt=False)),
             ("kind", dict(kind=2)), ("n_fam", dict(n_fam=-1))]
    before = c.untouched()
    for word, kw in cases:
        rc, got = c.run(p, **kw)
        msg = engine.lib.bsdc_last_error(engine.ctx).decode()
        assert rc == -22 and word in msg, (kw, rc, msg)
        for k in before:
            assert np.array_equal(got[k], before[k]), (kw, k)
    c.check(p, W.reference("reads", "M2_1_0"), "after the refusals")
