// cli zipper on the GPU (gfx950): the aligned consensus records with the tags of their unmapped
// partners put back, in coordinate order -- what `samtools sort -n | fgbio ZipperBams --sort
// Coordinate | samtools view -F 4` leaves (rules mergeAunA_consensus and
// mergeAunA_consensus_grepaligned, main.snake.py:97-119; rules in DESIGN.md section 3.11, these
// kernels in 8.12).  Two pieces, each with a host twin made of the same functions:
//
// bsdc_zip_sort: a stable LSD radix sort of 64-bit keys (refID << 32 | (pos + 1) << 1 | reverse)
// with a 32-bit payload, 8 bits a pass.  A pass whose digit is zero in every key (known from the
// largest refID and pos) is skipped.  A pass is five launches: k_zs_hist (a workgroup counts the
// digits of its tile of 2048 keys in LDS -> hist[digit][tile]), the offset scan of bsdc_devtext.h
// over hist in that order, and k_zs_scatter (a workgroup walks its tile again 256 keys at a time;
// a key's place = the scan's base of its digit and tile + the keys of that digit before it in the
// tile: counted per wavefront by ballots over the digit's bits, the wavefronts taking their turn
// in order at an LDS counter).  Keys and payload ping-pong between the caller's arrays and tmp.
//
// bsdc_zip_format: one wavefront per output record, in sorted order: k_zip_sizes, the offset scan,
// k_zip_write.  Every lane walks the two aux lists by type (the same walk in all lanes) to decide
// which tags stay and which are flipped; runs of tags that are copied as they are leave by
// "a lane owns one aligned destination dword" (funnel-shifted source dwords: bsdc_devtext.h load4 /
// can4; zp_copy keeps its own loop, which picks dword or bytes by the source too), a flipped Z or B
// payload by the lane that owns the destination byte / element.
// Bounds: a table entry that leaves the byte buffers makes a record of size 0 (the launcher
// refuses it from the host copy first); a sorted index >= n likewise; a walk stops at a tag that
// is unknown or leaves its aux block (the launcher refuses such records from the host copies, by
// name); no byte at or past `cap` is written.
//
// bsdc_zip_gather (cli zipper --stream true's merge rounds): output record k is source record
// order[k], unchanged: the offset scan over the table's lengths, then k_zip_gather, one wavefront
// per record with k_zip_write's copy (zp_copy_to).  An order entry >= n or a table entry that
// leaves src is a record of no bytes; the launcher refuses both from the host copies first.
// Built without hipcc this file holds the twins alone.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/bsdc.h"
#include "bsdc_auxwalk.h"  // zp_fixed, zp_tag_end, zp_name, zp_aux_error
#include "bsdc_devtext.h"

namespace {

using namespace bsdc_devtext;

constexpr int kZsBits = 8;                 // bits a pass
constexpr int kZsBins = 1 << kZsBits;
constexpr int kZsPasses = 64 / kZsBits;
constexpr int kZsThreads = 256;
constexpr int kZsPer = 8;                  // keys a thread
constexpr int kZsTile = kZsThreads * kZsPer;
constexpr int64_t kZipMaxRec = (int64_t)1 << 30;  // a record's bytes, both sides together
constexpr int kZipStat = 1;                // dwords per record in tmp: size

// ---- the sort ----

BSDC_HD uint32_t zs_digit(uint64_t key, int pass) { return (uint32_t)(key >> (kZsBits * pass)) & (kZsBins - 1); }

// the largest key of refID <= max_ref, pos <= max_pos
BSDC_HD uint64_t zs_max_key(int32_t max_ref, int32_t max_pos) {
    return (uint64_t)(uint32_t)max_ref << 32 | (uint64_t)((uint32_t)(max_pos + 1)) << 1 | 1u;
}
// a pass whose digit is zero in every key is skipped: the two halves of the key are bounded apart
BSDC_HD bool zs_pass_needed(int32_t max_ref, int32_t max_pos, int pass) {
    const uint64_t m = zs_max_key(max_ref, max_pos);
    const uint32_t half = pass < 4 ? (uint32_t)m : (uint32_t)(m >> 32);
    return (half >> (kZsBits * (pass & 3))) != 0;
}

// ---- the records ----

struct ZpArgs {
    const uint32_t *idx;
    const bsdc_zip_rec *tab;
    const uint8_t *rec, *part;
    int64_t rec_bytes, part_bytes;
    bsdc_zip_tags tags;
    int64_t n_fam;  // the records (the scan's name for its items)
    int64_t *off;
    uint8_t *dst;
    int64_t cap;
    int64_t *bsum;   // [groups + 1]
    uint32_t *stat;  // [n][kZipStat]
    int64_t groups;
};

BSDC_HD int64_t scan_bytes(const ZpArgs &A, int64_t r, int) { return (int64_t)A.stat[r * kZipStat]; }
BSDC_HD int64_t *scan_off(const ZpArgs &A, int) { return A.off; }

BSDC_HD bool zp_listed(const uint8_t *names, int n, uint8_t c0, uint8_t c1) {
    for (int k = 0; k < n; k++)
        if (names[2 * k] == c0 && names[2 * k + 1] == c1) return true;
    return false;
}
// a tag of this name occurs in the aux block (walked by type)
BSDC_HD bool zp_in_aux(const uint8_t *a, int64_t n, uint8_t c0, uint8_t c1) {
    for (int64_t i = 0; i < n;) {
        const int64_t j = zp_tag_end(a, i, n);
        if (j < 0) break;
        if (a[i] == c0 && a[i + 1] == c1) return true;
        i = j;
    }
    return false;
}
BSDC_HD uint8_t zp_comp(uint8_t c) {
    switch (c) {
    case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
    case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return c;
    }
}

// One output record.  Everything here is the same in every lane of its wavefront.
struct ZpRec {
    const uint8_t *r, *p;  // the aligned record (its block_size field), the partner's aux
    int64_t rn, ra, pn;    // the record's bytes, its aux start, the partner's aux bytes
    uint32_t flag;
};

BSDC_HD ZpRec zp_rec(const ZpArgs &A, int64_t k) {
    ZpRec q;
    const uint32_t s = A.idx[k];
    bsdc_zip_rec e;
    const bool in = (int64_t)s < A.n_fam;
    if (in) e = A.tab[s];
    const bool ok = in && e.rec_len >= 36 && e.aux_start >= 36 && e.aux_start <= e.rec_len && e.part_len >= 0 &&
                    (int64_t)e.rec_len + e.part_len <= kZipMaxRec && e.rec_off >= 0 && e.rec_off + e.rec_len <= A.rec_bytes &&
                    e.part_off >= 0 && e.part_off + e.part_len <= A.part_bytes;
    q.r = A.rec + (ok ? e.rec_off : 0);
    q.p = A.part + (ok ? e.part_off : 0);
    q.rn = ok ? e.rec_len : 0;
    q.ra = ok ? e.aux_start : 0;
    q.pn = ok ? e.part_len : 0;
    q.flag = ok ? (((uint32_t)q.r[18] | (uint32_t)q.r[19] << 8) & ~0x200u) | (e.flag_or & 0x200u) : 0;
    return q;
}

// byte i of the record's part before the aux: block_size and the flag are the output's
BSDC_HD uint8_t zp_head_byte(const ZpRec &q, uint32_t size, int64_t i) {
    if (i < 4) return (uint8_t)((size - 4) >> (8 * i));
    if (i == 18) return (uint8_t)q.flag;
    if (i == 19) return (uint8_t)(q.flag >> 8);
    return q.r[i];
}

// src[0 .. len) to dst + o, this lane's dwords; HEAD: the bytes are the record's first ones (zp_head_byte)
// (zp_copy_to: the same on any destination of `cap` writable bytes -- bsdc_zip_gather's copy too)
template <bool HEAD>
BSDC_HD void zp_copy_to(uint8_t *base, int64_t cap, const ZpRec &q, uint32_t size, const uint8_t *buf, int64_t buf_n,
                      const uint8_t *src, int64_t len, int64_t o, int lane, int nlanes) {
    const int ho = (int)((uintptr_t)(base + o) & 3u);
    const int64_t nd = (ho + len + 3) >> 2;
    for (int64_t k = lane; k < nd; k += nlanes) {
        const int64_t i0 = 4 * k - ho, p = o + i0;
        const bool patched = HEAD && (i0 < 4 || (i0 < 20 && i0 + 4 > 16));
        if (i0 >= 0 && i0 + 4 <= len && p + 4 <= cap && !patched && can4(buf, buf_n, src + i0)) {
            const uint32_t v = load4(src + i0);
            memcpy(__builtin_assume_aligned(base + p, 4), &v, 4);  // (aligned: one dword store)
            continue;
        }
        for (int b = 0; b < 4; b++) {
            const int64_t i = i0 + b;
            if (i >= 0 && i < len && p + b < cap) base[p + b] = HEAD ? zp_head_byte(q, size, i) : src[i];
        }
    }
}
template <bool HEAD>
BSDC_HD void zp_copy(const ZpArgs &A, const ZpRec &q, uint32_t size, const uint8_t *buf, int64_t buf_n, const uint8_t *src,
                   int64_t len, int64_t o, int lane, int nlanes) {
    zp_copy_to<HEAD>(A.dst, A.cap, q, size, buf, buf_n, src, len, o, lane, nlanes);
}

// what rule 5 does to a partner's tag of an output record with flag 0x10: 0 nothing, 1 reversed, 2 reverse-complemented
BSDC_HD int zp_mode(const ZpArgs &A, const uint8_t *t) {
    const bool rv = zp_listed(A.tags.reverse, A.tags.n_reverse, t[0], t[1]);
    if (t[2] == 'B') return rv ? 1 : 0;
    if (t[2] != 'Z') return 0;
    return rv ? 1 : zp_listed(A.tags.revcomp, A.tags.n_revcomp, t[0], t[1]) ? 2 : 0;
}

// the tag t[0 .. len) flipped to dst + o: a lane writes the destination bytes (Z) or elements (B) it owns
BSDC_HD void zp_flip(const ZpArgs &A, const uint8_t *t, int64_t len, int mode, int64_t o, int lane, int nlanes) {
    uint8_t *base = A.dst;
    if (t[2] == 'Z') {
        const int64_t m = len - 4;  // the string without its NUL
        for (int64_t i = lane; i < len; i += nlanes) {
            uint8_t c = t[i];
            if (i >= 3 && i < 3 + m) {
                c = t[3 + (m - 1 - (i - 3))];
                if (mode == 2) c = zp_comp(c);
            }
            if (o + i < A.cap) base[o + i] = c;
        }
        return;
    }
    const int es = zp_fixed(t[3]);
    const int64_t cnt = (len - 8) / es;
    for (int64_t i = lane; i < 8; i += nlanes)
        if (o + i < A.cap) base[o + i] = t[i];
    for (int64_t e = lane; e < cnt; e += nlanes)
        for (int b = 0; b < es; b++) {
            const int64_t i = 8 + e * es + b;
            if (o + i < A.cap) base[o + i] = t[8 + (cnt - 1 - e) * es + b];
        }
}

// The record at dst + o (WRITE) -> its size.  `size`: what the size pass gave (the block_size field).
template <bool WRITE>
BSDC_HD int64_t zp_emit(const ZpArgs &A, const ZpRec &q, uint32_t size, int64_t o, int lane, int nlanes) {
    if (q.rn == 0) return 0;
    int64_t w = q.ra;
    if (WRITE) zp_copy<true>(A, q, size, A.rec, A.rec_bytes, q.r, q.ra, o, lane, nlanes);
    // the aligned record's tags that the partner does not carry and that are not removed, in runs
    const uint8_t *ax = q.r + q.ra;
    const int64_t an = q.rn - q.ra;
    int64_t run = 0, run_len = 0;
    for (int64_t i = 0; i < an;) {
        const int64_t j = zp_tag_end(ax, i, an);
        if (j < 0) break;
        const bool keep = !zp_listed(A.tags.remove, A.tags.n_remove, ax[i], ax[i + 1]) && !zp_in_aux(q.p, q.pn, ax[i], ax[i + 1]);
        if (keep) {
            if (!run_len) run = i;
            run_len += j - i;
        }
        if (!keep || j == an) {
            if (WRITE && run_len) zp_copy<false>(A, q, size, A.rec, A.rec_bytes, ax + run, run_len, o + w, lane, nlanes);
            w += run_len;
            run_len = 0;
        }
        i = j;
    }
    if (run_len) {  // (the walk stopped at a malformed tag)
        if (WRITE) zp_copy<false>(A, q, size, A.rec, A.rec_bytes, ax + run, run_len, o + w, lane, nlanes);
        w += run_len;
        run_len = 0;
    }
    // the partner's tags that are not removed; of a reverse record, the listed ones flipped
    const bool rev = (q.flag & 0x10u) != 0;
    for (int64_t i = 0; i < q.pn;) {
        const int64_t j = zp_tag_end(q.p, i, q.pn);
        if (j < 0) break;
        const bool keep = !zp_listed(A.tags.remove, A.tags.n_remove, q.p[i], q.p[i + 1]);
        const int mode = keep && rev ? zp_mode(A, q.p + i) : 0;
        if (keep && !mode) {
            if (!run_len) run = i;
            run_len += j - i;
        }
        if (!keep || mode || j == q.pn) {
            if (WRITE && run_len) zp_copy<false>(A, q, size, A.part, A.part_bytes, q.p + run, run_len, o + w, lane, nlanes);
            w += run_len;
            run_len = 0;
        }
        if (mode) {
            if (WRITE) zp_flip(A, q.p + i, j - i, mode, o + w, lane, nlanes);
            w += j - i;
        }
        i = j;
    }
    if (run_len) {
        if (WRITE) zp_copy<false>(A, q, size, A.part, A.part_bytes, q.p + run, run_len, o + w, lane, nlanes);
        w += run_len;
    }
    return w;
}

thread_local std::string g_zp_err;

int32_t zp_fail(const std::string &m) {
    g_zp_err = m;
    return BSDC_EINVAL;
}

int64_t zp_bound(const bsdc_zip_rec *tab, int64_t n) {
    if (n < 0 || (n && !tab)) return -1;
    int64_t s = 0;
    for (int64_t k = 0; k < n; k++) {
        if (tab[k].rec_len < 0 || tab[k].part_len < 0) return -1;
        s += (int64_t)tab[k].rec_len + tab[k].part_len;
    }
    return s;
}

// the arguments, as the launcher and the twin both refuse them (host copies of tab, rec, part); fills A
int32_t zp_check(const char *who, const uint32_t *idx, int64_t n, const bsdc_zip_rec *dev_tab, const bsdc_zip_rec *tab,
                 const uint8_t *rec, const uint8_t *rec_host, int64_t rec_bytes, const uint8_t *part, const uint8_t *part_host,
                 int64_t part_bytes, const bsdc_zip_tags *tags, int64_t *off, uint8_t *dst, int64_t cap, ZpArgs *A) {
    const std::string w(who);
    if (n < 0 || n > (int64_t)1 << 30) return zp_fail(w + ": n is negative or beyond 2^30");
    if (rec_bytes < 0 || part_bytes < 0) return zp_fail(w + ": a negative byte count");
    if (!idx) return zp_fail(w + ": idx is null");
    if (!dev_tab || !tab) return zp_fail(w + ": tab is null");
    if (!rec || !rec_host) return zp_fail(w + ": rec is null");
    if (!part || !part_host) return zp_fail(w + ": part is null");
    if (!tags) return zp_fail(w + ": tags is null");
    if (!off) return zp_fail(w + ": off is null");
    if (!dst) return zp_fail(w + ": dst is null");
    if (tags->n_reverse < 0 || tags->n_reverse > BSDC_ZIP_MAX_TAGS || tags->n_revcomp < 0 || tags->n_revcomp > BSDC_ZIP_MAX_TAGS ||
        tags->n_remove < 0 || tags->n_remove > BSDC_ZIP_MAX_TAGS)
        return zp_fail(w + ": a tag list of more than " + std::to_string(BSDC_ZIP_MAX_TAGS) + " names");
    if (((uintptr_t)rec & 3u) || ((uintptr_t)part & 3u) || ((uintptr_t)idx & 3u))
        return zp_fail(w + ": rec, part and idx must be 4-byte aligned");
    if (((uintptr_t)off & 7u) || ((uintptr_t)dev_tab & 7u)) return zp_fail(w + ": off and tab must be 8-byte aligned");
    for (int64_t k = 0; k < n; k++) {
        const bsdc_zip_rec &e = tab[k];
        const char *bad = nullptr;
        if (e.rec_len < 36 || e.aux_start < 36 || e.aux_start > e.rec_len) bad = "rec_len or aux_start outside the record";
        else if (e.rec_off < 0 || e.rec_off + e.rec_len > rec_bytes) bad = "its bytes leave rec";
        else if (e.part_len < 0 || e.part_off < 0 || e.part_off + e.part_len > part_bytes) bad = "its partner's aux bytes leave part";
        else if ((int64_t)e.rec_len + e.part_len > kZipMaxRec) bad = "more than 2^30 bytes";
        if (bad) return zp_fail(w + ": record " + std::to_string(k) + ": " + bad);
        std::string m = zp_aux_error(rec_host + e.rec_off + e.aux_start, e.rec_len - e.aux_start);
        if (m.empty()) m = zp_aux_error(part_host + e.part_off, e.part_len);
        if (!m.empty())
            return zp_fail(w + ": record " + std::to_string(k) + " (read " + zp_name(rec_host + e.rec_off, e.rec_len) + "): " + m);
    }
    const int64_t need = zp_bound(tab, n);
    if (need < 0 || cap < need)
        return zp_fail(w + ": cap " + std::to_string(cap) + " is below bsdc_zip_bytes_bound " + std::to_string(need));
    A->idx = idx, A->tab = dev_tab, A->rec = rec, A->part = part, A->rec_bytes = rec_bytes, A->part_bytes = part_bytes;
    A->tags = *tags;
    A->n_fam = n, A->off = off, A->dst = dst, A->cap = cap;
    A->bsum = nullptr, A->stat = nullptr, A->groups = 0;
    return 0;
}

int32_t zs_check(const char *who, const uint64_t *keys, const uint32_t *idx, int64_t n, int32_t max_ref, int32_t max_pos) {
    const std::string w(who);
    if (n < 0 || n > (int64_t)1 << 30) return zp_fail(w + ": n is negative or beyond 2^30");
    if (!keys || !idx) return zp_fail(w + ": keys or idx is null");
    if (max_ref < 0 || max_pos < -1 || max_pos > 0x7ffffffe) return zp_fail(w + ": max_ref or max_pos is out of range");
    if (((uintptr_t)keys & 7u) || ((uintptr_t)idx & 3u)) return zp_fail(w + ": keys must be 8-byte and idx 4-byte aligned");
    return 0;
}

// ---- the gather (cli zipper --stream's merge rounds) ----

struct ZgArgs {
    const uint32_t *order;
    const int64_t *src_off;
    const int32_t *src_len;
    const uint8_t *src;
    int64_t src_bytes;
    int64_t n_fam;  // the records (the scan's name for its items)
    int64_t *off;
    uint8_t *dst;
    int64_t cap;
    int64_t *bsum;  // [groups + 1]
    int64_t groups;
};

// output record k: its source bytes; an order entry >= n or an entry that leaves src is a record of no bytes
BSDC_HD int64_t zg_rec(const ZgArgs &A, int64_t k, const uint8_t **from) {
    const uint32_t s = A.order[k];
    if ((int64_t)s >= A.n_fam) return 0;
    const int64_t o = A.src_off[s], n = A.src_len[s];
    if (n <= 0 || n > kZipMaxRec || o < 0 || o + n > A.src_bytes) return 0;
    *from = A.src + o;
    return n;
}
BSDC_HD int64_t scan_bytes(const ZgArgs &A, int64_t k, int) {
    const uint8_t *from;
    return zg_rec(A, k, &from);
}
BSDC_HD int64_t *scan_off(const ZgArgs &A, int) { return A.off; }

BSDC_HD void zg_copy(const ZgArgs &A, int64_t k, int64_t o, int lane, int nlanes) {
    const uint8_t *from = A.src;
    const int64_t n = zg_rec(A, k, &from);
    if (n) zp_copy_to<false>(A.dst, A.cap, ZpRec(), 0, A.src, A.src_bytes, from, n, o, lane, nlanes);
}

// the arguments, as the launcher and the twin both refuse them (host copies of order, src_off, src_len); fills A
int32_t zg_check(const char *who, const uint32_t *order, const uint32_t *order_host, int64_t n, const int64_t *src_off,
                 const int64_t *src_off_host, const int32_t *src_len, const int32_t *src_len_host, const uint8_t *src,
                 int64_t src_bytes, int64_t *off, uint8_t *dst, int64_t cap, ZgArgs *A) {
    const std::string w(who);
    if (n < 0 || n > (int64_t)1 << 30) return zp_fail(w + ": n is negative or beyond 2^30");
    if (src_bytes < 0 || cap < 0) return zp_fail(w + ": a negative byte count");
    if (!order || !order_host) return zp_fail(w + ": order is null");
    if (!src_off || !src_off_host || !src_len || !src_len_host) return zp_fail(w + ": src_off or src_len is null");
    if (!src) return zp_fail(w + ": src is null");
    if (!off) return zp_fail(w + ": off is null");
    if (!dst) return zp_fail(w + ": dst is null");
    if (((uintptr_t)src & 3u) || ((uintptr_t)dst & 3u) || ((uintptr_t)order & 3u) || ((uintptr_t)src_len & 3u))
        return zp_fail(w + ": src, dst, order and src_len must be 4-byte aligned");
    if (((uintptr_t)off & 7u) || ((uintptr_t)src_off & 7u)) return zp_fail(w + ": off and src_off must be 8-byte aligned");
    for (int64_t k = 0; k < n; k++) {
        const int64_t o = src_off_host[k], len = src_len_host[k];
        if (len < 0 || len > kZipMaxRec || o < 0 || o + len > src_bytes)
            return zp_fail(w + ": record " + std::to_string(k) + ": its bytes leave src");
    }
    int64_t need = 0;
    for (int64_t k = 0; k < n; k++) {
        if ((int64_t)order_host[k] >= n) return zp_fail(w + ": order[" + std::to_string(k) + "] is not below n");
        need += src_len_host[order_host[k]];
    }
    if (cap < need) return zp_fail(w + ": cap " + std::to_string(cap) + " is below the records' bytes " + std::to_string(need));
    A->order = order, A->src_off = src_off, A->src_len = src_len, A->src = src, A->src_bytes = src_bytes;
    A->n_fam = n, A->off = off, A->dst = dst, A->cap = cap, A->bsum = nullptr, A->groups = 0;
    return 0;
}

#ifdef __HIPCC__
struct ZsArgs {
    const uint64_t *kin;
    const uint32_t *vin;
    uint64_t *kout;
    uint32_t *vout;
    int64_t n, tiles;
    int pass;
    uint32_t *hist;  // [kZsBins][tiles]
    int64_t n_fam;   // kZsBins * tiles (the scan's items)
    int64_t *off;    // [n_fam + 1]
    int64_t *bsum;
    int64_t groups;
};
BSDC_HD int64_t scan_bytes(const ZsArgs &A, int64_t i, int) { return (int64_t)A.hist[i]; }
BSDC_HD int64_t *scan_off(const ZsArgs &A, int) { return A.off; }

__global__ __launch_bounds__(kZsThreads) void k_zs_hist(ZsArgs A) {
    __shared__ uint32_t h[kZsBins];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kZsTile;
    for (int j = 0; j < kZsPer; j++) {
        const int64_t i = base + j * kZsThreads + t;
        if (i < A.n) atomicAdd(&h[zs_digit(A.kin[i], A.pass)], 1u);
    }
    __syncthreads();
    A.hist[(int64_t)t * A.tiles + blockIdx.x] = h[t];
}

__global__ __launch_bounds__(kZsThreads) void k_zs_scatter(ZsArgs A) {
    __shared__ uint32_t cnt[kZsBins];   // the tile's keys of each digit placed so far
    __shared__ int64_t first[kZsBins];  // where the tile's keys of each digit start
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    cnt[t] = 0;
    first[t] = A.off[(int64_t)t * A.tiles + blockIdx.x];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kZsTile;
    for (int j = 0; j < kZsPer; j++) {
        const int64_t i = base + j * kZsThreads + t;
        const bool valid = i < A.n;
        const uint64_t key = valid ? A.kin[i] : 0;
        const uint32_t val = valid ? A.vin[i] : 0;
        const uint32_t d = zs_digit(key, A.pass);
        // the lanes of this wavefront that hold a key of the same digit
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < kZsBits; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const int lead = valid && peers ? __ffsll((long long)peers) - 1 : lane;
        const uint32_t before = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        uint32_t rank = 0;
        for (int w = 0; w < kZsThreads / 64; w++) {  // the wavefronts in order: the scatter is stable
            if (wave == w) {
                uint32_t old = 0;
                if (valid && lane == lead) old = atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
                rank = (uint32_t)__shfl((int)old, lead) + before;
            }
            __syncthreads();
        }
        if (valid) {
            const int64_t p = first[d] + rank;
            if (p >= 0 && p < A.n) {
                A.kout[p] = key;
                A.vout[p] = val;
            }
        }
    }
}

__global__ __launch_bounds__(kT) void k_zip_sizes(ZpArgs A) {
    const int64_t k = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= A.n_fam) return;
    const ZpRec q = zp_rec(A, k);
    const int64_t size = zp_emit<false>(A, q, 0, 0, 0, 64);
    if ((threadIdx.x & 63) == 0) A.stat[k * kZipStat] = (uint32_t)size;
}

__global__ __launch_bounds__(kT) void k_zip_write(ZpArgs A) {
    const int64_t k = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= A.n_fam) return;
    const ZpRec q = zp_rec(A, k);
    zp_emit<true>(A, q, A.stat[k * kZipStat], A.off[k], threadIdx.x & 63, 64);
}

// one wavefront per output record, as k_zip_write: a lane owns one aligned destination dword at a time
__global__ __launch_bounds__(kT) void k_zip_gather(ZgArgs A) {
    const int64_t k = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= A.n_fam) return;
    zg_copy(A, k, A.off[k], threadIdx.x & 63, 64);
}

int64_t zs_tiles(int64_t n) { return (n + kZsTile - 1) / kZsTile; }
int64_t zs_groups(int64_t n) { return (zs_tiles(n) * kZsBins + kFamPerGroup - 1) / kFamPerGroup; }
int64_t zp_groups(int64_t n) { return (n + kFamPerGroup - 1) / kFamPerGroup; }
#endif

}  // namespace

extern "C" {

const char *bsdc_zip_last_error(void) { return g_zp_err.c_str(); }

int32_t bsdc_zip_sort_tile(void) { return kZsTile; }

int64_t bsdc_zip_bytes_bound(const bsdc_zip_rec *tab_host, int64_t n) { return zp_bound(tab_host, n); }

int64_t bsdc_zip_scan_host(const uint8_t *bytes, int64_t n_bytes, bsdc_zip_src *out, int64_t cap) {
    if (!bytes || n_bytes < 0 || cap < 0) return zp_fail("bsdc_zip_scan_host: a null or negative argument");
    int64_t n = 0;
    for (int64_t p = 0; p < n_bytes; n++) {
        const std::string at = "bsdc_zip_scan_host: record " + std::to_string(n);
        if (p + 36 > n_bytes) return zp_fail(at + ": truncated");
        const uint8_t *r = bytes + p;
        int32_t f[9];
        memcpy(f, r, 36);
        const int64_t bs = f[0];
        const int l_name = r[12], n_cig = (int)((uint32_t)f[4] & 0xffffu);
        const int64_t l_seq = f[5];
        const int64_t body = 36 + (int64_t)l_name + 4 * (int64_t)n_cig + (l_seq + 1) / 2 + l_seq;
        if (bs < 32 || p + 4 + bs > n_bytes) return zp_fail(at + ": truncated");
        if (l_seq < 0 || l_name < 2 || body > 4 + bs || 4 + bs > kZipMaxRec) return zp_fail(at + ": malformed lengths");
        if (out && n < cap) {
            bsdc_zip_src &e = out[n];
            e.off = p, e.len = (int32_t)(4 + bs), e.aux = (int32_t)body, e.ref_id = f[1], e.pos = f[2];
            e.flag = (uint16_t)((uint32_t)f[4] >> 16), e.name_len = (uint8_t)(l_name - 1), e.reserved0 = 0, e.reserved = 0;
        }
        p += 4 + bs;
    }
    return n;
}

int64_t bsdc_zip_scan_prefix_host(const uint8_t *bytes, int64_t n_bytes, bsdc_zip_src *out, int64_t cap, int64_t *consumed) {
    if (!bytes || n_bytes < 0 || cap < 0 || !consumed) return zp_fail("bsdc_zip_scan_prefix_host: a null or negative argument");
    int64_t n = 0, p = 0;
    for (; p + 36 <= n_bytes; n++) {
        const std::string at = "bsdc_zip_scan_prefix_host: record " + std::to_string(n);
        const uint8_t *r = bytes + p;
        int32_t f[9];
        memcpy(f, r, 36);
        const int64_t bs = f[0];
        const int l_name = r[12], n_cig = (int)((uint32_t)f[4] & 0xffffu);
        const int64_t l_seq = f[5];
        const int64_t body = 36 + (int64_t)l_name + 4 * (int64_t)n_cig + (l_seq + 1) / 2 + l_seq;
        // (the fixed fields are all there: lengths that leave the record are an error, cut or not)
        if (bs < 32 || l_seq < 0 || l_name < 2 || body > 4 + bs || 4 + bs > kZipMaxRec) return zp_fail(at + ": malformed lengths");
        if (p + 4 + bs > n_bytes) break;  // the cut record: the caller's carry
        if (out && n < cap) {
            bsdc_zip_src &e = out[n];
            e.off = p, e.len = (int32_t)(4 + bs), e.aux = (int32_t)body, e.ref_id = f[1], e.pos = f[2];
            e.flag = (uint16_t)((uint32_t)f[4] >> 16), e.name_len = (uint8_t)(l_name - 1), e.reserved0 = 0, e.reserved = 0;
        }
        p += 4 + bs;
    }
    *consumed = p;
    return n;
}

int32_t bsdc_zip_gather_host(const uint32_t *order, int64_t n, const int64_t *src_off, const int32_t *src_len, const uint8_t *src,
                             int64_t src_bytes, int64_t *off, uint8_t *dst, int64_t cap) {
    ZgArgs A;
    if (const int32_t rc = zg_check("bsdc_zip_gather_host", order, order, n, src_off, src_off, src_len, src_len, src, src_bytes,
                                    off, dst, cap, &A))
        return rc;
    int64_t o = 0;
    for (int64_t k = 0; k < n; k++) {
        off[k] = o;
        zg_copy(A, k, o, 0, 1);
        o += scan_bytes(A, k, 0);
    }
    off[n] = o;
    return 0;
}

int32_t bsdc_zip_sort_host(uint64_t *keys, uint32_t *idx, int64_t n, int32_t max_ref, int32_t max_pos) {
    if (const int32_t rc = zs_check("bsdc_zip_sort_host", keys, idx, n, max_ref, max_pos)) return rc;
    std::vector<uint64_t> k2((size_t)n);
    std::vector<uint32_t> v2((size_t)n);
    uint64_t *ka = keys, *kb = k2.data();
    uint32_t *va = idx, *vb = v2.data();
    for (int pass = 0; pass < kZsPasses; pass++) {
        if (!zs_pass_needed(max_ref, max_pos, pass)) continue;
        int64_t at[kZsBins + 1] = {0};
        for (int64_t i = 0; i < n; i++) at[zs_digit(ka[i], pass) + 1]++;
        for (int d = 0; d < kZsBins; d++) at[d + 1] += at[d];
        for (int64_t i = 0; i < n; i++) {
            const int64_t p = at[zs_digit(ka[i], pass)]++;
            kb[p] = ka[i], vb[p] = va[i];
        }
        std::swap(ka, kb), std::swap(va, vb);
    }
    if (ka != keys && n) {
        memcpy(keys, ka, (size_t)n * sizeof(uint64_t));
        memcpy(idx, va, (size_t)n * sizeof(uint32_t));
    }
    return 0;
}

int32_t bsdc_zip_format_host(const uint32_t *idx, int64_t n, const bsdc_zip_rec *tab, const uint8_t *rec, int64_t rec_bytes,
                             const uint8_t *part, int64_t part_bytes, const bsdc_zip_tags *tags, int64_t *off, uint8_t *dst,
                             int64_t cap) {
    ZpArgs A;
    if (const int32_t rc = zp_check("bsdc_zip_format_host", idx, n, tab, tab, rec, rec, rec_bytes, part, part, part_bytes, tags,
                                    off, dst, cap, &A))
        return rc;
    for (int64_t k = 0; k < n; k++)
        if ((int64_t)idx[k] >= n) return zp_fail("bsdc_zip_format_host: idx[" + std::to_string(k) + "] is not below n");
    int64_t o = 0;
    for (int64_t k = 0; k < n; k++) {
        const ZpRec q = zp_rec(A, k);
        const int64_t size = zp_emit<false>(A, q, 0, 0, 0, 1);
        off[k] = o;
        zp_emit<true>(A, q, (uint32_t)size, o, 0, 1);
        o += size;
    }
    off[n] = o;
    return 0;
}

#ifdef __HIPCC__
int64_t bsdc_zip_sort_tmp_bytes(int64_t n) {
    if (n < 0) return -1;
    const int64_t items = zs_tiles(n) * kZsBins;
    return n * 8 + (items + 1) * 8 + (zs_groups(n) + 1) * 8 + n * 4 + items * 4 + 8;
}

int32_t bsdc_zip_sort(uint64_t *keys, uint32_t *idx, int64_t n, int32_t max_ref, int32_t max_pos, uint8_t *tmp, void *stream) {
    if (const int32_t rc = zs_check("bsdc_zip_sort", keys, idx, n, max_ref, max_pos)) return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return zp_fail("bsdc_zip_sort: tmp is null or not 8-byte aligned");
    if (n == 0) return 0;
    ZsArgs A;
    A.n = n, A.tiles = zs_tiles(n), A.n_fam = A.tiles * kZsBins, A.groups = zs_groups(n);
    uint64_t *k2 = reinterpret_cast<uint64_t *>(tmp);
    A.off = reinterpret_cast<int64_t *>(tmp + n * 8);
    A.bsum = A.off + A.n_fam + 1;
    uint32_t *v2 = reinterpret_cast<uint32_t *>(A.bsum + A.groups + 1);
    A.hist = v2 + n;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *ka = keys, *kb = k2;
    uint32_t *va = idx, *vb = v2;
    for (int pass = 0; pass < kZsPasses; pass++) {
        if (!zs_pass_needed(max_ref, max_pos, pass)) continue;
        A.kin = ka, A.vin = va, A.kout = kb, A.vout = vb, A.pass = pass;
        hipLaunchKernelGGL(k_zs_hist, dim3((unsigned)A.tiles), dim3(kZsThreads), 0, st, A);
        launch_scan<1>(A, st);
        hipLaunchKernelGGL(k_zs_scatter, dim3((unsigned)A.tiles), dim3(kZsThreads), 0, st, A);
        std::swap(ka, kb), std::swap(va, vb);
    }
    hipError_t e = hipSuccess;
    if (ka != keys) {
        e = hipMemcpyAsync(keys, ka, (size_t)n * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(idx, va, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
    }
    if (hipGetLastError() != hipSuccess || e != hipSuccess) {
        g_zp_err = "bsdc_zip_sort: a kernel launch or copy failed";
        return BSDC_EDEVICE;
    }
    return 0;
}

int64_t bsdc_zip_format_tmp_bytes(int64_t n) {
    if (n < 0) return -1;
    return (zp_groups(n) + 1) * (int64_t)sizeof(int64_t) + n * kZipStat * (int64_t)sizeof(uint32_t) + 8;
}

int32_t bsdc_zip_format(const uint32_t *idx, int64_t n, const bsdc_zip_rec *tab, const bsdc_zip_rec *tab_host,
                        const uint8_t *rec, const uint8_t *rec_host, int64_t rec_bytes, const uint8_t *part,
                        const uint8_t *part_host, int64_t part_bytes, const bsdc_zip_tags *tags, int64_t *off, uint8_t *dst,
                        int64_t cap, uint8_t *tmp, void *stream) {
    ZpArgs A;
    if (const int32_t rc = zp_check("bsdc_zip_format", idx, n, tab, tab_host, rec, rec_host, rec_bytes, part, part_host,
                                    part_bytes, tags, off, dst, cap, &A))
        return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return zp_fail("bsdc_zip_format: tmp is null or not 8-byte aligned");
    A.groups = zp_groups(n);
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    A.stat = reinterpret_cast<uint32_t *>(tmp + (A.groups + 1) * sizeof(int64_t));
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)((n + kT / 64 - 1) / (kT / 64));
    if (wgs) hipLaunchKernelGGL(k_zip_sizes, dim3(wgs), dim3(kT), 0, st, A);
    launch_scan<1>(A, st);
    if (wgs) hipLaunchKernelGGL(k_zip_write, dim3(wgs), dim3(kT), 0, st, A);
    if (hipGetLastError() != hipSuccess) {
        g_zp_err = "bsdc_zip_format: a kernel launch failed";
        return BSDC_EDEVICE;
    }
    return 0;
}

int64_t bsdc_zip_gather_tmp_bytes(int64_t n) {
    if (n < 0) return -1;
    return (zp_groups(n) + 1) * (int64_t)sizeof(int64_t) + 8;
}

int32_t bsdc_zip_gather(const uint32_t *order, const uint32_t *order_host, int64_t n, const int64_t *src_off,
                        const int64_t *src_off_host, const int32_t *src_len, const int32_t *src_len_host, const uint8_t *src,
                        int64_t src_bytes, int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream) {
    ZgArgs A;
    if (const int32_t rc = zg_check("bsdc_zip_gather", order, order_host, n, src_off, src_off_host, src_len, src_len_host, src,
                                    src_bytes, off, dst, cap, &A))
        return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return zp_fail("bsdc_zip_gather: tmp is null or not 8-byte aligned");
    A.groups = zp_groups(n);
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)((n + kT / 64 - 1) / (kT / 64));
    launch_scan<1>(A, st);
    if (wgs) hipLaunchKernelGGL(k_zip_gather, dim3(wgs), dim3(kT), 0, st, A);
    if (hipGetLastError() != hipSuccess) {
        g_zp_err = "bsdc_zip_gather: a kernel launch failed";
        return BSDC_EDEVICE;
    }
    return 0;
}
#endif

}  // extern "C"
