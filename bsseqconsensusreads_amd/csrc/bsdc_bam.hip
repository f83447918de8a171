// BAM record emission on the GPU (gfx950): the output BAM's records of a batch's kept families --
// block_size, the fixed fields, name, packed SEQ, QUAL, the family's aux bytes (RG / MI / RX) and
// fgbio's consensus tags -- written in HBM from the consensus and the single-strand rows where the
// vote (and the filter) left them, so that with bsdc_bgzf_crc32 and bsdc_bgzf.hip's deflate only
// compressed blocks cross PCIe (include/bsdc.h).  The bytes are those of
// libbsdc_io's encode_records over bam.duplex_records' records with bsdc_consensus_tags' aux.
//
// bsdc_bam_format, five launches on one stream, no host step between them:
//  1. k_bam_sizes: one wavefront per output record (family f, end e).  A record's size depends on
//     its depths (an integer tag takes the smallest BAM type), so the reductions come first: lanes
//     stride over the record's columns, max / min / sum of depth and sum of errors of the duplex
//     ("c"), "a" and "b" reads are reduced over the wave, and the up to nine results (xD, xM, the
//     bits of xE) and the record's size land in `tmp`, 12 dwords a record;
//  2-4. the offset scan of bsdc_devtext.h over the families' byte counts -> off[f];
//  5. k_bam_write: one wavefront per record.  A record starts at any byte, so a lane owns one
//     ALIGNED dword of the destination at a time (bsdc_devtext.h store_record), assembles its four
//     bytes in a register and stores it whole; only a record's first and last partial dword (and a
//     dword that would cross `cap`) leave as single bytes.  A dword inside QUAL, packed SEQ, a B:s array, ac / bc or
//     aq / bq is made of aligned source dwords (load4, nt16x4, add33x4); the fixed fields, the
//     names, the aux, the tag heads and the seams go byte by byte.
// The rows a / b of a record, the duplex column rule and xE are bsdc_ssrows.h's.
// xE = (float)sum(err) / (float)sum(depth): exact 64-bit sums, one rounding each in the
// conversions, an IEEE divide (this file is built without fast-math); the 0 / 0 of a read without
// depth takes the bits the launcher computed on the host, which are what the host encoder writes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"
#include "bsdc_ssrows.h"

namespace {

using namespace bsdc_devtext;

constexpr int kMaxName = 253;           // l_read_name <= 254 (encode_records)
constexpr int64_t kMaxAux = 1 << 20;    // a family's aux bytes (RG / MI / RX: tens of bytes)
constexpr int kStat = 12;               // dwords per record in tmp: size, cD cM cE, aD aM aE, bD bM bE, 2 spare

struct BmArgs {
    const uint8_t *status;
    const uint16_t *len;
    const uint8_t *seq;
    const uint8_t *qual;
    const uint8_t *filt;
    const int64_t *name_off;
    const uint8_t *name_buf;
    const int64_t *aux_off;
    const uint8_t *aux_buf;
    const uint16_t *ss_len;
    const uint8_t *ss_base, *ss_qual, *ss_depth, *ss_err;
    const int32_t *ss_wide;
    const uint16_t *ss_wdepth, *ss_werr;
    int64_t n_fam;
    int32_t stride, kind, with_tags;
    uint32_t nan_bits;
    int64_t *off;
    uint8_t *rec;
    int64_t cap;
    int64_t *bsum;   // [groups + 1]
    uint32_t *stat;  // [2 * n_fam][kStat]
    int64_t groups;
};

BSDC_HD bool bm_kept(const BmArgs &A, int64_t f) { return (A.status[f] & 1) && (A.filt == nullptr || A.filt[f] == 0); }
BSDC_HD int bm_len(const BmArgs &A, int64_t f, int e) {
    const int l = A.len[2 * f + e];
    return l < A.stride ? l : A.stride;  // (a row holds stride bases: no read past it whatever len says)
}
BSDC_HD int bm_table_len(const int64_t *off, int64_t f, int64_t hi) {
    const int64_t n = off[f + 1] - off[f];
    return n < 0 ? 0 : n > hi ? (int)hi : (int)n;  // (the host checked its copy)
}
BSDC_HD int64_t scan_bytes(const BmArgs &A, int64_t f, int) {
    return (int64_t)A.stat[(2 * f) * kStat] + (int64_t)A.stat[(2 * f + 1) * kStat];
}
BSDC_HD int64_t *scan_off(const BmArgs &A, int) { return A.off; }

// one single-strand read's rows, cut to the record's length by the caller
using bsdc_ssrows::Row;
// b when sb, else a, field by field (registers stay registers)
BSDC_HD Row ss_pick(bool sb, const Row &a, const Row &b) {
    return Row{sb ? b.b : a.b, sb ? b.q : a.q, sb ? b.d8 : a.d8, sb ? b.e8 : a.e8, sb ? b.d16 : a.d16, sb ? b.e16 : a.e16};
}
// xD, xM and the bits of xE of one read; a record's: the duplex ("c"), "a" and "b" reads'
struct Trip {
    uint32_t D, M, E;
};
struct Stats {
    Trip c, a, b;
};

// row (f, s) of the single-strand outputs (on: else an empty view, nothing read)
BSDC_HD Row bm_view(const BmArgs &A, bool on, int64_t f, int s) {
    if (!on) return Row{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return bsdc_ssrows::row_of(A, f, s, A.ss_wide ? A.ss_wide[f] : -1);
}

// One record (family f, end e).  Everything here is the same in every lane of its wavefront.
struct BmRec {
    const uint8_t *nm, *ax, *sq, *ql;
    int nl, al, L, e;
    int tags, kind, two;  // tags: the consensus tags follow; two: the "b" read is present (duplex)
    Row a, b;
    int o_seq, o_qual, o_aux, o_tags;  // where the sections start in the record
};

// the record without its tag statistics; its size up to the tags (o_tags)
BSDC_HD BmRec bm_rec(const BmArgs &A, int64_t f, int e) {
    BmRec r;
    r.nm = A.name_buf + A.name_off[f];
    r.ax = A.aux_buf + A.aux_off[f];
    r.sq = A.seq + (2 * f + e) * (int64_t)(A.stride / 2);
    r.ql = A.qual + (2 * f + e) * (int64_t)A.stride;
    r.nl = bm_table_len(A.name_off, f, kMaxName);
    r.al = bm_table_len(A.aux_off, f, kMaxAux);
    r.L = bm_len(A, f, e);
    r.e = e;
    r.tags = A.with_tags;
    r.kind = A.kind;
    // (without tags: the molecular selection, which reads nothing)
    const bsdc_ssrows::End s = bsdc_ssrows::end_rows(r.tags ? r.kind : 1, A.ss_len, f, e);
    r.two = s.two;
    r.a = bm_view(A, r.tags != 0, f, s.a);
    r.b = bm_view(A, s.two, f, s.b);
    r.o_seq = 36 + r.nl + 1;
    r.o_qual = r.o_seq + (r.L + 1) / 2;
    r.o_aux = r.o_qual + r.L;
    r.o_tags = r.o_aux + r.al;
    return r;
}

// ---- the tags' bytes ----

// an integer tag: 'x' 'y' type value, the smallest BAM type that holds v (v >= 0)
BSDC_HD int int_size(uint32_t v) { return v > 65535u ? 7 : v > 255u ? 5 : 4; }
BSDC_HD uint32_t int_byte(uint32_t x, uint32_t y, uint32_t v, int t) {
    if (t == 0) return x;
    if (t == 1) return y;
    if (t == 2) return v > 65535u ? 'I' : v > 255u ? 'S' : 'C';
    return (v >> (8 * (t - 3))) & 0xffu;
}
// xD xM xE of one read
BSDC_HD int trip_size(const Trip &p) { return int_size(p.D) + int_size(p.M) + 7; }
BSDC_HD uint32_t trip_byte(uint32_t x, const Trip &p, int t) {
    int s = int_size(p.D);
    if (t < s) return int_byte(x, 'D', p.D, t);
    t -= s;
    s = int_size(p.M);
    if (t < s) return int_byte(x, 'M', p.M, t);
    t -= s;
    if (t == 0) return x;
    if (t == 1) return 'E';
    if (t == 2) return 'f';
    return (p.E >> (8 * (t - 3))) & 0xffu;
}
// a B:s array 'x' 'y' 'B' 's' count values: 8 + 2 L bytes; the bytes widened, or the u16 values as they are
BSDC_HD uint32_t arr_byte(uint32_t x, uint32_t y, const uint8_t *v8, const uint16_t *v16, int L, int t) {
    if (t == 0) return x;
    if (t == 1) return y;
    if (t == 2) return 'B';
    if (t == 3) return 's';
    if (t < 8) return ((uint32_t)L >> (8 * (t - 4))) & 0xffu;
    const int k = t - 8;
    if (v16) return ((uint32_t)v16[k >> 1] >> (8 * (k & 1))) & 0xffu;
    return (k & 1) ? 0u : (uint32_t)v8[k >> 1];
}
// bytes k .. k + 3 of an array's 2 L value bytes (all four inside them)
BSDC_HD uint32_t arr_dword(const uint8_t *v8, const uint16_t *v16, int k) {
    if (v16) return load4(reinterpret_cast<const uint8_t *>(v16) + k);
    const int j = (k + 1) >> 1;  // the first value whose low byte lies in the dword
    return (k & 1) ? (uint32_t)v8[j] << 8 | (uint32_t)v8[j + 1] << 24 : (uint32_t)v8[j] | (uint32_t)v8[j + 1] << 16;
}
// a Z tag of L mapped bytes: 'x' 'y' 'Z' bytes NUL: 4 + L bytes
BSDC_HD uint32_t text_byte(uint32_t x, uint32_t y, const uint8_t *v, bool nt16, int L, int t) {
    if (t == 0) return x;
    if (t == 1) return y;
    if (t == 2) return 'Z';
    const int k = t - 3;
    if (k >= L) return 0;
    return nt16 ? nt16x4((uint32_t)v[k] & 15u) & 0xffu : ((uint32_t)v[k] + 33u) & 0xffu;
}

// sizes of the tag sections of a record with statistics st
BSDC_HD int bm_trips(const BmRec &r, const Stats &st) {
    if (r.kind == 1) return trip_size(st.c);
    return trip_size(st.c) + trip_size(st.a) + (r.two ? trip_size(st.b) : 0);
}
BSDC_HD int bm_strand(const BmRec &r) { return 24 + 6 * r.L; }  // xd xe xc xq of one strand
BSDC_HD int bm_arrays(const BmRec &r) { return r.kind == 1 ? 16 + 4 * r.L : bm_strand(r) * (r.two ? 2 : 1); }

// byte t of the tags (0 <= t < their size)
BSDC_HD uint32_t tag_byte(const BmRec &r, const Stats &st, int t) {
    int s = trip_size(st.c);
    if (t < s) return trip_byte('c', st.c, t);
    t -= s;
    const int L = r.L;
    if (r.kind == 1) {
        if (t < 8 + 2 * L) return arr_byte('c', 'd', r.a.d8, r.a.d16, L, t);
        return arr_byte('c', 'e', r.a.e8, r.a.e16, L, t - (8 + 2 * L));
    }
    s = trip_size(st.a);
    if (t < s) return trip_byte('a', st.a, t);
    t -= s;
    if (r.two) {
        s = trip_size(st.b);
        if (t < s) return trip_byte('b', st.b, t);
        t -= s;
    }
    const bool sb = t >= bm_strand(r);
    if (sb) t -= bm_strand(r);
    const Row v = ss_pick(sb, r.a, r.b);
    const uint32_t x = sb ? 'b' : 'a';
    if (t < 8 + 2 * L) return arr_byte(x, 'd', v.d8, v.d16, L, t);
    t -= 8 + 2 * L;
    if (t < 8 + 2 * L) return arr_byte(x, 'e', v.e8, v.e16, L, t);
    t -= 8 + 2 * L;
    if (t < 4 + L) return text_byte(x, 'c', v.b, true, L, t);
    return text_byte(x, 'q', v.q, false, L, t - (4 + L));
}

// dword w of the record's first 36 bytes: block_size, then the 32 fixed bytes of an unmapped
// paired record (tid -1, pos -1, l_read_name, mapq 0, bin 4680, no cigar, flag, l_seq, next -1 / -1, tlen 0)
BSDC_HD uint32_t fixed_dword(const BmRec &r, int size, int w) {
    switch (w) {
    case 0: return (uint32_t)(size - 4);
    case 3: return (uint32_t)(r.nl + 1) | 4680u << 16;
    case 4: return (r.e ? 141u : 77u) << 16;
    case 5: return (uint32_t)r.L;
    case 8: return 0u;
    default: return 0xffffffffu;  // 1, 2: tid, pos; 6, 7: next tid, next pos
    }
}

// byte i of the record (0 outside it)
BSDC_HD uint32_t bm_byte(const BmRec &r, const Stats &st, int size, int i) {
    if (i < 0 || i >= size) return 0;
    if (i < 36) return (fixed_dword(r, size, i >> 2) >> (8 * (i & 3))) & 0xffu;
    if (i < r.o_seq) return i - 36 < r.nl ? (uint32_t)r.nm[i - 36] : 0u;
    if (i < r.o_qual) {
        const int j = i - r.o_seq;
        const uint32_t b = r.sq[j];
        return 2 * j + 1 < r.L ? b : b & 0xf0u;  // (the pad nibble of an odd length is 0)
    }
    if (i < r.o_aux) return r.ql[i - r.o_qual];
    if (i < r.o_tags) return r.ax[i - r.o_aux];
    return tag_byte(r, st, i - r.o_tags);
}

// bytes i0 .. i0 + 3 of the record as one little-endian dword (bytes outside the record: 0)
BSDC_HD uint32_t bm_dword(const BmRec &r, const Stats &st, int size, int o_arr, int i0) {
    const int L = r.L;
    if (i0 >= r.o_qual && i0 + 4 <= r.o_aux) return load4(r.ql + (i0 - r.o_qual));
    if (i0 >= r.o_seq && i0 + 4 <= r.o_seq + L / 2) return load4(r.sq + (i0 - r.o_seq));  // (whole bytes only)
    if (r.tags && i0 >= o_arr && i0 + 4 <= size) {
        int t = i0 - o_arr;
        const bool sb = r.kind == 0 && t >= bm_strand(r);
        if (sb) t -= bm_strand(r);
        const Row v = ss_pick(sb, r.a, r.b);
        int k = t - 8;
        if (k >= 0 && k + 4 <= 2 * L) return arr_dword(v.d8, v.d16, k);
        k = t - (16 + 2 * L);
        if (k >= 0 && k + 4 <= 2 * L) return arr_dword(v.e8, v.e16, k);
        if (r.kind == 0) {
            k = t - (19 + 4 * L);
            if (k >= 0 && k + 4 <= L) return nt16x4(load4(v.b + k) & 0x0f0f0f0fu);
            k = t - (23 + 5 * L);
            if (k >= 0 && k + 4 <= L) return add33x4(load4(v.q + k));
        }
    }
    uint32_t x = 0;
    for (int b = 0; b < 4; b++) x |= bm_byte(r, st, size, i0 + b) << (8 * b);
    return x;
}

// D, M, the bits of E of one read from its lanes' partial results
__device__ __forceinline__ Trip read_stats(uint32_t mx, uint32_t mn, uint64_t sd, uint64_t se, int L, uint32_t nan_bits) {
    mx = wave_max(mx);
    mn = wave_min(mn);
    sd = wave_sum(sd);
    se = wave_sum(se);
    const float q = bsdc_ssrows::read_rate((int64_t)se, (int64_t)sd);
    return Trip{mx, L ? mn : 0u, (sd == 0 && se == 0) ? nan_bits : __float_as_uint(q)};
}

__global__ __launch_bounds__(kT) void k_bam_sizes(BmArgs A) {
    const int64_t w = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int64_t f = w >> 1;
    const int e = (int)(w & 1);
    if (f >= A.n_fam) return;
    const int lane = threadIdx.x & 63;
    uint32_t *out = A.stat + w * kStat;
    if (!bm_kept(A, f)) {
        if (lane == 0) out[0] = 0;
        return;
    }
    const BmRec r = bm_rec(A, f, e);
    Stats st{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int size = r.o_tags;
    if (r.tags) {
        uint32_t cmx = 0, cmn = 0xffffffffu, amx = 0, amn = 0xffffffffu, bmx = 0, bmn = 0xffffffffu;
        uint64_t csd = 0, cse = 0, asd = 0, ase = 0, bsd = 0, bse = 0;
        for (int i = lane; i < r.L; i += 64) {
            const uint32_t ad = r.a.d(i), ae = r.a.e(i);
            amx = ad > amx ? ad : amx;
            amn = ad < amn ? ad : amn;
            asd += ad;
            ase += ae;
            uint32_t cd = ad, ce = ae;
            if (r.two) {
                const uint32_t bd = r.b.d(i), be = r.b.e(i);
                bmx = bd > bmx ? bd : bmx;
                bmn = bd < bmn ? bd : bmn;
                bsd += bd;
                bse += be;
                const bsdc_ssrows::Col c = bsdc_ssrows::duplex_col(r.a.b[i], r.a.q[i], ad, ae, r.b.b[i], r.b.q[i], bd, be);
                cd = c.d;
                ce = c.e;
            }
            cmx = cd > cmx ? cd : cmx;
            cmn = cd < cmn ? cd : cmn;
            csd += cd;
            cse += ce;
        }
        st.c = read_stats(cmx, cmn, csd, cse, r.L, A.nan_bits);
        if (r.kind == 0) {
            st.a = read_stats(amx, amn, asd, ase, r.L, A.nan_bits);
            if (r.two) st.b = read_stats(bmx, bmn, bsd, bse, r.L, A.nan_bits);
        }
        size += bm_trips(r, st) + bm_arrays(r);
    }
    if (lane < 10) {  // (selects: no runtime-indexed register array)
        const uint32_t v = lane == 0 ? (uint32_t)size : lane == 1 ? st.c.D : lane == 2 ? st.c.M : lane == 3 ? st.c.E :
                           lane == 4 ? st.a.D : lane == 5 ? st.a.M : lane == 6 ? st.a.E :
                           lane == 7 ? st.b.D : lane == 8 ? st.b.M : st.b.E;
        out[lane] = v;
    }
}

__global__ __launch_bounds__(kT) void k_bam_write(BmArgs A) {
    const int64_t w = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int64_t f = w >> 1;
    const int e = (int)(w & 1);
    if (f >= A.n_fam || !bm_kept(A, f)) return;
    const uint32_t *in = A.stat + w * kStat;
    const int size = (int)in[0];
    const Stats st{{in[1], in[2], in[3]}, {in[4], in[5], in[6]}, {in[7], in[8], in[9]}};
    const BmRec r = bm_rec(A, f, e);
    const int o_arr = r.o_tags + (r.tags ? bm_trips(r, st) : 0);
    const int64_t o = A.off[f] + (e ? (int64_t)A.stat[(2 * f) * kStat] : 0);
    store_record(A.rec, o, size, A.cap, threadIdx.x & 63, 64, [&](int i0) { return bm_dword(r, st, size, o_arr, i0); });
}

int64_t groups_of(int64_t n_fam) { return (n_fam + kFamPerGroup - 1) / kFamPerGroup; }

}  // namespace

extern "C" {

int64_t bsdc_bam_bytes_bound(int64_t n_fam, int64_t name_bytes, int64_t aux_bytes, int32_t stride, int32_t kind,
                             int32_t with_tags) {
    if (n_fam < 0 || name_bytes < 0 || aux_bytes < 0 || stride < 0 || kind < 0 || kind > 1) return -1;
    // a record: block_size, 32 fixed bytes, name NUL, packed SEQ, QUAL, aux; tags at their largest
    // (I integers; both strands): kind 1 cD cM cE cd ce, kind 0 three reads' D M E and two strands' d e c q
    int64_t per = 36 + 1 + (stride + 1) / 2 + (int64_t)stride;
    if (with_tags) per += kind == 1 ? 21 + 2 * (8 + 2 * (int64_t)stride) : 3 * 21 + 2 * (24 + 6 * (int64_t)stride);
    return 2 * (n_fam * per + name_bytes + aux_bytes);
}

int64_t bsdc_bam_tmp_bytes(int64_t n_fam) {
    if (n_fam < 0) return -1;
    return (groups_of(n_fam) + 1) * (int64_t)sizeof(int64_t) + 2 * n_fam * kStat * (int64_t)sizeof(uint32_t);
}

int32_t bsdc_bam_format(const bsdc_consensus *out, const uint8_t *filt, int32_t kind, int32_t with_tags, int64_t n_fam,
                        const int64_t *name_off, const uint8_t *name_buf, const int64_t *name_off_host,
                        const int64_t *aux_off, const uint8_t *aux_buf, const int64_t *aux_off_host, int64_t *off,
                        uint8_t *rec, int64_t cap, uint8_t *tmp, void *stream) {
    if (!out || !out->status || !out->len || !out->seq || !out->qual || !name_off || !name_buf || !name_off_host ||
        !aux_off || !aux_buf || !aux_off_host || !off || !rec || !tmp)
        return BSDC_EINVAL;
    if (kind < 0 || kind > 1 || n_fam < 0 || n_fam > (int64_t)1 << 30 || cap < 0 || out->stride <= 0 ||
        out->stride % 16 != 0)
        return BSDC_EINVAL;
    if (with_tags) {
        if (!out->ss_len || !out->ss_base || !out->ss_qual || !out->ss_depth || !out->ss_err) return BSDC_EINVAL;
        if (out->ss_wide && (!out->ss_wdepth || !out->ss_werr)) return BSDC_EINVAL;
        if (((uintptr_t)out->ss_base & 3u) || ((uintptr_t)out->ss_qual & 3u) || ((uintptr_t)out->ss_wdepth & 3u) ||
            ((uintptr_t)out->ss_werr & 3u))
            return BSDC_EINVAL;
    }
    if (((uintptr_t)out->seq & 3u) || ((uintptr_t)out->qual & 3u) || ((uintptr_t)tmp & 7u) || ((uintptr_t)off & 7u))
        return BSDC_EINVAL;
    for (int64_t f = 0; f < n_fam; f++) {
        const int64_t nl = name_off_host[f + 1] - name_off_host[f], al = aux_off_host[f + 1] - aux_off_host[f];
        if (nl < 0 || nl > kMaxName || al < 0 || al > kMaxAux) return BSDC_EINVAL;
    }
    volatile float zero = 0.0f;  // the host's own 0 / 0: what the host encoder writes for a read without depth
    const float nan = zero / zero;
    BmArgs A;
    memcpy(&A.nan_bits, &nan, 4);
    A.status = out->status;
    A.len = out->len;
    A.seq = out->seq;
    A.qual = out->qual;
    A.filt = filt;
    A.name_off = name_off;
    A.name_buf = name_buf;
    A.aux_off = aux_off;
    A.aux_buf = aux_buf;
    A.ss_len = out->ss_len;
    A.ss_base = out->ss_base;
    A.ss_qual = out->ss_qual;
    A.ss_depth = out->ss_depth;
    A.ss_err = out->ss_err;
    A.ss_wide = out->ss_wide;
    A.ss_wdepth = out->ss_wdepth;
    A.ss_werr = out->ss_werr;
    A.n_fam = n_fam;
    A.stride = out->stride;
    A.kind = kind;
    A.with_tags = with_tags ? 1 : 0;
    A.off = off;
    A.rec = rec;
    A.cap = cap;
    A.groups = groups_of(n_fam);
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    A.stat = reinterpret_cast<uint32_t *>(tmp + (A.groups + 1) * sizeof(int64_t));
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)((2 * n_fam + kT / 64 - 1) / (kT / 64));
    if (wgs) hipLaunchKernelGGL(k_bam_sizes, dim3(wgs), dim3(kT), 0, st, A);
    launch_scan<1>(A, st);
    if (wgs) hipLaunchKernelGGL(k_bam_write, dim3(wgs), dim3(kT), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : BSDC_EDEVICE;
}

}  // extern "C"
