"""Shared test helpers: golden fixtures and record comparisons."""
import gzip
import json
import os

import numpy as np

from bsseqconsensusreads_amd import records as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as fh:
        return json.load(fh)


def golden_inputs(g):
    raw = R.records_from_dicts(g["input"])
    names = [c["name"] for c in g["header"]["references"]]
    ref = R.Reference.from_contigs(names, g["contigs"], header_lengths=[c["length"] for c in g["header"]["references"]])
    return raw, ref


def compare_records(golden_out, produced, raw, inputs, what=""):
    """golden_out: list of fixture dicts (reference tool output, in order);
    produced: an OracleRecords / OutRecords with .record(k); inputs: fixture input dicts."""
    n = len(produced.src)
    assert n == len(golden_out), "%s: %d records vs golden %d" % (what, n, len(golden_out))
    for k in range(n):
        g = golden_out[k]
        p = produced.record(k)
        src = inputs[p["src"]]
        ctx = "%s record %d (%s flag %d)" % (what, k, g["name"], g["flag"])
        assert src["name"] == g["name"] and src["flag"] == g["flag"], ctx + ": wrong record/order"
        assert p["pos"] == g["pos"], ctx + ": pos %d vs %d" % (p["pos"], g["pos"])
        gc = [(l << 4) | op for op, l in g["cigar"]]
        assert [int(x) for x in p["cigar"]] == gc, ctx + ": cigar %s vs %s" % (
            R.cigar_string(p["cigar"]), R.cigar_string(gc))
        gs = R.encode_seq(g["seq"]) if g["seq"] else np.zeros(0, np.uint8)
        assert np.array_equal(p["seq"], gs), ctx + ": seq\n%s\n%s" % (R.decode_seq(p["seq"]), g["seq"])
        gq = np.frombuffer(g["qual"].encode(), np.uint8) - 33 if g["qual"] is not None else None
        assert gq is not None and np.array_equal(p["qual"], gq), ctx + ": qual"
        gt = {t[0]: t[2] for t in g["tags"]}
        st = {t[0]: t[2] for t in src["tags"]}
        for t in ("RD", "LA"):
            exp = gt.get(t, None)
            got = p[t.lower()] if p[t.lower()] >= 0 else st.get(t, None)
            assert exp == got, ctx + ": tag %s %r vs %r" % (t, got, exp)
        # every other tag passes through
        assert {k: v for k, v in gt.items() if k not in ("RD", "LA")} == {k: v for k, v in st.items() if k not in ("RD", "LA")}, ctx


def trim_tails(raw, frac=0.3, seed=1, min_len=30):
    """Adapter-trimmed reads: a fraction of records lose a random number of 3' bases (sequencing
    orientation: the end of a forward read, the start of a reverse one), cigar and position
    adjusted.  Simple-cigar records only; others pass unchanged."""
    rng = np.random.default_rng(seed)
    b = R._Builder()
    for k in range(raw.n):
        seq, qual = raw.record_seq(k).copy(), raw.record_qual(k).copy()
        cig = [int(x) for x in raw.record_cigar(k)]
        flag, pos, L = int(raw.flag[k]), int(raw.pos[k]), len(seq)
        if len(cig) == 1 and (cig[0] & 0xF) == R.OP_M and L > min_len and rng.random() < frac:
            cut = int(rng.integers(1, L - min_len))
            if flag & 16:  # reverse read: its 3' end is the leftmost bases
                seq, qual, pos = seq[cut:], qual[cut:], pos + cut
            else:
                seq, qual = seq[:L - cut], qual[:L - cut]
            cig = [((L - cut) << 4) | R.OP_M]
        tags = [("MI", "Z", "%s/%s" % (raw.mi_id[k], "A" if raw.mi_strand[k] == 0 else "B")),
                ("MC", "Z", "%dM" % L)]
        b.add(("t%d" % raw.name_id[k]).encode(), flag, int(raw.tid[k]), pos, 60, cig, seq, qual,
              int(raw.next_tid[k]), int(raw.next_pos[k]), int(raw.tlen[k]), R.encode_aux(tags), tags)
    return b.finish()


def near_tie_votes(raw, n_pos=6, seed=3, qlo=80, qhi=93, p_n=0.1, n_alleles=2):
    """Adversarial vote columns (a copy of `raw`): per family, `n_pos` reference positions inside
    its forward reads' span get, in every record covering them, a random A/C/G/T base (`n_alleles`
    alleles per position) at a random quality in [qlo, qhi] (an N at Q2 with probability p_n).  High
    qualities make the per-read likelihoods nearly equal (lr[q] saturates at the post-UMI error
    rate), so columns where the bases disagree are near ties -- fgbio's fp64 sums separate them,
    2^-20 fixed point does not."""
    import dataclasses
    rng = np.random.default_rng(seed)
    seq, qual = raw.seq.copy(), raw.qual.copy()
    pos = raw.pos.astype(np.int64)
    fam = raw.mi_id.astype(np.int64)
    L = raw.l_seq.astype(np.int64)
    fwd = (raw.flag & 16) == 0
    n_fam = int(fam.max()) + 1 if raw.n else 0
    start = np.full(n_fam, np.iinfo(np.int64).max)
    np.minimum.at(start, fam[fwd], pos[fwd])
    P = start[:, None] + rng.integers(20, 130, size=(n_fam, n_pos))
    alle = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=(n_fam, n_pos, n_alleles))
    for k in range(raw.n):
        f = int(fam[k])
        j = P[f] - pos[k]
        ok = (j >= 0) & (j < L[k])
        for i in np.nonzero(ok)[0]:
            o = int(raw.seq_off[k] + j[i])
            if rng.random() < p_n:
                seq[o], qual[o] = 15, 2
            else:
                seq[o] = alle[f, i, int(rng.integers(0, n_alleles))]
                qual[o] = int(rng.integers(qlo, qhi + 1))
    return dataclasses.replace(raw, seq=seq, qual=qual)


def gpu_vs_fp64(engine, raw, ref, run_tools, what, molecular=False, pre=45.0, post=30.0, min_cbq=None,
                overlap=True, dump=False):
    """One GPU run against both references: oracle/ bit for bit (consensus, single-strand reads,
    tag statistics) and the fp64 restatement of fgbio (tests/fgbio_vote.py) within the fp64 bar
    (test_fgbio_vote.assert_fp64_bar), single-strand and duplex.  The engine runs with the given
    flags for this call only; min_cbq defaults to the caller's own (0 molecular, 2 duplex).
    dump (step 5 with the tools): also fetch the tool-2 records.
    -> (Consensus, compare_ss counts, tool-2 records or None, OracleResult)."""
    import fgbio_vote as fv
    from bsseqconsensusreads_amd import pipeline
    from oracle import oracle
    from test_fgbio_vote import assert_fp64_bar
    from test_gpu_parity import assert_consensus_equal, assert_ss_equal
    engine.load_reference(ref)
    if min_cbq is None:
        min_cbq = 0 if molecular else 2  # main.snake.py:54 vs the duplex caller's single-strand caller
    t2 = None
    with engine.flags(error_rate_pre_umi=pre, error_rate_post_umi=post, consensus_call_overlapping_bases=overlap,
                      min_consensus_base_quality=min_cbq):
        if molecular:
            cons, raw = pipeline.run_molecular(engine, raw, tags=True, min_consensus_base_quality=min_cbq)
            r = oracle.run(raw, ref, pre=pre, post=post, overlap=overlap, keep_sources=True, run_tools=False,
                           family_order="mi-group", min_consensus_base_quality=min_cbq)
        else:
            if run_tools:
                cons, t2 = pipeline.run_step5(engine, raw, dump=dump, tags=True)
            else:
                cons = pipeline.run_duplex(engine, raw, tags=True)
            r = oracle.run(raw, ref, pre=pre, post=post, overlap=overlap, keep_sources=True, run_tools=run_tools,
                           min_consensus_base_quality=min_cbq)
    assert_consensus_equal(cons, r, what)      # GPU == fixed-point restatement, bit for bit
    assert_ss_equal(cons, r, what)
    src = r.sources
    stride = cons.ss["base"].shape[2]
    ss = fv.ss_vote(src["count"], src["len"], src["base"], src["qual"], stride, pre=pre, post=post, min_cbq=min_cbq)
    em = np.nonzero((cons.status & 1) != 0)[0]  # (the kernels' single-strand reads: emitted families)
    c = fv.compare_ss({"len": cons.ss["len"][em], "base": cons.ss["base"][em], "qual": cons.ss["qual"][em]},
                      {k: v[em] for k, v in ss.items()})
    assert_fp64_bar(c, what)
    # duplex consensus vs fgbio fp64 duplex of the fp64 single-strand reads
    st, ln, b, q = fv.duplex(ss)
    assert np.array_equal(st, (cons.status & 1).astype(np.int32)) and np.array_equal(ln, cons.length)
    w = min(b.shape[2], cons.seq.shape[2])
    live = np.arange(w)[None, None, :] < ln[:, :, None]
    db = live & (cons.seq[:, :, :w] != b[:, :, :w])
    dq = np.abs(cons.qual[:, :, :w].astype(np.int64) - q[:, :, :w].astype(np.int64))
    print(what, "duplex columns %d, base diffs %d, qual +-1 %d, qual >1 %d" % (
        int(live.sum()), int(db.sum()), int((live & (dq == 1)).sum()), int((live & (dq > 1)).sum())))
    # a duplex column can differ only where one of its single-strand inputs does (a +-1 qual); with
    # none of those (the usual case), the duplex reads are identical
    same = np.ones(b.shape, bool)
    for e, (sa, sb) in enumerate(((0, 3), (1, 2))):
        for st_ in (sa, sb):
            same[:, e, :w] &= (cons.ss["base"][:, st_, :w] == ss["base"][:, st_, :w]) & \
                              (cons.ss["qual"][:, st_, :w] == ss["qual"][:, st_, :w])
    same[(cons.status & 1) == 0] = True  # (no duplex read there: ln is 0)
    assert not (db & same[:, :, :w]).any(), what + ": duplex base differs from fgbio fp64"
    assert not (live & (dq > 0) & same[:, :, :w]).any(), what + ": duplex qual differs from fgbio fp64"
    if c["qual_pm1"] == 0 and c["n_boundary"] == 0:
        assert int(db.sum()) == 0 and int((live & (dq > 0)).sum()) == 0
    return cons, c, t2, r


def assert_bam_matches_oracle(out_bam, in_bam, fasta, what=""):
    """The step-5 output BAM, record by record (R1, R2 per emitted family, TemplateCoordinate
    order): name suffix, SEQ and QUAL against oracle/ on the whole input file."""
    from bsseqconsensusreads_amd import bam
    from oracle import oracle
    _, whole = bam.read_bam(in_bam, threads=4)
    ref = bam.read_fasta(fasta, bam.read_bam_header(in_bam))
    r = oracle.run(whole, ref, threads=8)
    em = np.nonzero(r.status == 1)[0]
    _, out = bam.read_bam(out_bam, threads=4)
    assert out.n == 2 * em.shape[0], "%s: %d records vs %d" % (what, out.n, 2 * em.shape[0])
    for j, f in enumerate(em):
        mi = whole.mi_names[int(r.fam_mi[f])]
        mi = mi if isinstance(mi, bytes) else mi.encode()
        for e in range(2):
            k = 2 * j + e
            n = int(r.cons_len[f, e])
            ctx = "%s family %d end %d" % (what, f, e)
            assert int(out.l_seq[k]) == n, ctx
            assert np.array_equal(out.record_seq(k), r.cons_seq[f, e, :n]), ctx + ": SEQ"
            assert np.array_equal(out.record_qual(k), r.cons_qual[f, e, :n]), ctx + ": QUAL"
            assert out.qname(k).endswith(b":" + mi), ctx + ": name"
    return int(out.n)
