// The rows of one output record (family f, end e) of a BSDC_MODE_TAGS run and the per-read values
// made from them: the one statement of DESIGN.md section 3.8 that the tag encoder (bsdc_io.cpp
// bsdc_consensus_tags), the BAM pass (bsdc_bam.hip), the filter (bsdc_filter.hip) and the metrics
// (bsdc_metrics.hip) share.  Plain C++17: host and device under hipcc, inline under g++.  How a
// caller walks its columns (8 a lane, 4 a lane, 1 a lane, sequentially) is its own business; the
// rules here work on values in registers.  fgbio parity of the duplex rule: PARITY UNPINNED.
// (bsdc_metrics.hip met_record writes duplex_col out once more, for its kernel's speed: a change
// of the rule goes there too.)
#ifndef BSDC_SSROWS_H
#define BSDC_SSROWS_H
#include <stdint.h>

#include "bsdc_devtext.h"  // BSDC_HD

namespace bsdc_ssrows {

// one single-strand row (f, s): bases, qualities, and the depths / errors as the kernels' bytes or,
// for a family with a wide row, as its exact u16 values (d16 / e16 set)
struct Row {
    const uint8_t *b, *q, *d8, *e8;
    const uint16_t *d16, *e16;
    BSDC_HD uint32_t d(int i) const { return d16 ? (uint32_t)d16[i] : (uint32_t)d8[i]; }
    BSDC_HD uint32_t e(int i) const { return e16 ? (uint32_t)e16[i] : (uint32_t)e8[i]; }
};

// row (f, s) of A's ss_* buffers (A: anything with ss_base, ss_qual, ss_depth, ss_err, ss_wdepth,
// ss_werr and stride); wide: the family's row in the wide table, -1 for none
template <class Args>
BSDC_HD Row row_of(const Args &A, int64_t f, int s, int32_t wide) {
    const size_t at = (size_t)(4 * f + s) * (size_t)A.stride;
    Row r{A.ss_base + at, A.ss_qual + at, A.ss_depth + at, A.ss_err + at, nullptr, nullptr};
    if (wide >= 0) {
        const size_t aw = (size_t)(4 * (int64_t)wide + s) * (size_t)A.stride;
        r.d16 = A.ss_wdepth + aw;
        r.e16 = A.ss_werr + aw;
    }
    return r;
}

// the strand rows of end e: a, b and whether b is read (two)
struct End {
    int a, b;
    bool two;
};
// molecular (kind 1): row e, no b (ss_len is not read).  duplex (kind 0): strand rows (0, 3) for R1
// and (1, 2) for R2; a = the AB row or the only one present
BSDC_HD End end_rows(int kind, const uint16_t *ss_len, int64_t f, int e) {
    End s{e, 3 - e, false};
    if (kind == 0) {
        const bool la = ss_len[4 * f + s.a] > 0, lb = ss_len[4 * f + s.b] > 0;
        s.two = la && lb;
        if (!la) s.a = s.b;
    }
    return s;
}

// one duplex column's depth and errors
struct Col {
    uint32_t d, e;
};
// the duplex call before its N mask; errors counted against it: a strand whose call agrees
// contributes its errors, one that disagrees all of its reads
BSDC_HD Col duplex_col(uint32_t ab, uint32_t aq, uint32_t ad, uint32_t ae, uint32_t bb, uint32_t bq, uint32_t bd,
                       uint32_t be) {
    const uint32_t x = ab & 15u, y = bb & 15u;
    const uint32_t raw = x == y ? x : aq > bq ? x : bq > aq ? y : x;
    return Col{ad + bd, (x == raw ? ae : ad) + (y == raw ? be : bd)};
}

// xE of one read: an IEEE float32 divide of the two sums, each converted as its own type (NaN at
// 0 / 0, +inf at n / 0)
template <class T>
BSDC_HD float read_rate(T err, T depth) {
    return (float)err / (float)depth;
}

}  // namespace bsdc_ssrows
#endif
