// The tool-stage records as BAM records on the GPU (gfx950): every record of a family batch after
// tool 1 and tool 2 -- what rule groupsort_convert leaves for fgbio CallDuplexConsensusReads
// (main.snake.py:144-153) -- written in HBM from the stage dump of a bsdc_run(.. | BSDC_MODE_DUMP)
// and a per-record table of the input record's own fields (include/bsdc.h bsdc_toolrec_rec; rules
// in DESIGN.md section 3.10, this kernel in 8.11).  Output record r is batch record r: the
// families in the step's order, the records of a family in the batch's.
//
// bsdc_toolrec_format, five launches on one stream, no host step between them:
//  1. k_toolrec_sizes: one wavefront per record.  Lanes stride over the record's cigar ops and the
//     reference length of the NEW cigar (the prepended / appended 1M, the op RD trims) is reduced
//     over the wave; the record's size and its bin (htslib's reg2bin) land in `tmp`, 2 dwords a record;
//  2-4. the offset scan of bsdc_devtext.h over the records' byte counts -> off[r];
//  5. k_toolrec_write: one wavefront per record.  A record starts at any byte, so a lane owns one
//     ALIGNED dword of the destination at a time (bsdc_devtext.h store_record), assembles its four
//     bytes in a register and stores it whole; only a record's first and last partial dword (and a
//     dword that would cross `cap`) leave as single bytes.  A dword inside QUAL, packed SEQ or the
//     aux bytes is made of aligned source dwords by a funnel shift (load4, tr_pack4); the fixed fields, the name,
//     the cigar, the RD / LA tags and the seams go byte by byte.
// Bounds: a record whose table entry leaves the name / cigar / aux buffers has size 0 (the launcher
// refuses such a table from the caller's host copy before anything runs); a record whose dump
// slot leaves the dump buffers has l_seq 0 in the kernel, which reads nothing there (rec[] and
// dump_len lie in HBM, out of the launcher's reach: the twin, which can read them, refuses, and
// Engine.toolrec checks the batch's slots against n_dump); no byte at or past `cap` is written.
// The per-record functions are __host__ __device__: bsdc_toolrec_host runs them sequentially on
// the CPU with one "lane"; built without hipcc this file holds that twin alone
// (tests/sanitize/toolrec_twin_main.cpp).
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"

namespace {

using namespace bsdc_devtext;

constexpr int kTrMaxName = 254;           // l_read_name <= 255 with its NUL
constexpr int kTrMaxCig = 65533;          // + the prepended and the appended 1M: n_cigar_op <= 65535
constexpr int64_t kTrMaxAux = 1 << 24;    // one record's aux bytes
constexpr int kTrStat = 2;                // dwords per record in tmp: size, bin
constexpr uint32_t kOp1M = 1u << 4;       // 1M

struct TrArgs {
    const int32_t *dump_pos;
    const uint16_t *dump_len;
    const uint8_t *dump_tags, *dump_seq, *dump_qual;
    const uint32_t *rec;  // [4 * n_rec]: rec[4 r] = the record's offset in dump_seq / dump_qual
    const bsdc_toolrec_rec *tab;
    const uint8_t *names;
    const uint32_t *cigar;
    const uint8_t *aux;
    int64_t n_fam;  // the records (the scan's name for its items)
    int64_t n_dump, name_bytes, n_ops, aux_bytes;
    int64_t *off;
    uint8_t *dst;
    int64_t cap;
    int64_t *bsum;   // [groups + 1]
    uint32_t *stat;  // [n_rec][kTrStat]
    int64_t groups;
};

BSDC_HD int64_t scan_bytes(const TrArgs &A, int64_t r, int) { return (int64_t)A.stat[r * kTrStat]; }
BSDC_HD int64_t *scan_off(const TrArgs &A, int) { return A.off; }

// four nt16 codes, one per byte -> two packed bytes (high nibble first)
BSDC_HD uint32_t tr_pack4(uint32_t x) {
    return ((x & 0xfu) << 4) | ((x >> 8) & 0xfu) | ((x >> 12) & 0xf0u) << 8 | ((x >> 24) & 0xfu) << 8;
}

// htslib's reg2bin over [beg, end)
BSDC_HD uint32_t tr_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14)) & 0xffffu;
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17)) & 0xffffu;
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20)) & 0xffffu;
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23)) & 0xffffu;
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26)) & 0xffffu;
    return 0;
}

// One record.  Everything here is the same in every lane of its wavefront.
struct TrRec {
    const uint8_t *nm, *ax, *sq, *ql;
    const uint32_t *cg;
    int32_t ref_id, pos, next_ref_id, next_pos, tlen;
    uint32_t flag, mapq, rd;
    int ok, nl, al, L, conv;  // conv: bit1, the RD / LA tags follow the aux
    int n, pre, body, dec, nc;  // cigar: input ops, prepended 1M, ops before the appended 1M, RD shortens the last, ops out
    int o_cig, o_seq, o_qual, o_aux, o_tags, size;
};

BSDC_HD TrRec tr_rec(const TrArgs &A, int64_t r) {
    TrRec q;
    const bsdc_toolrec_rec e = A.tab[r];
    q.ok = e.name_len >= 1 && e.name_len <= kTrMaxName && e.name_off >= 0 && e.name_off + e.name_len <= A.name_bytes &&
           e.n_cig >= 0 && e.n_cig <= kTrMaxCig && e.cig_off >= 0 && e.cig_off + e.n_cig <= A.n_ops &&
           e.aux_len >= 0 && e.aux_len <= kTrMaxAux && e.aux_off >= 0 && e.aux_off + e.aux_len <= A.aux_bytes;
    q.nl = q.ok ? e.name_len : 0;
    q.al = q.ok ? e.aux_len : 0;
    q.n = q.ok ? e.n_cig : 0;
    q.nm = A.names + (q.ok ? e.name_off : 0);
    q.ax = A.aux + (q.ok ? e.aux_off : 0);
    q.cg = A.cigar + (q.ok ? e.cig_off : 0);
    q.ref_id = e.ref_id, q.next_ref_id = e.next_ref_id, q.next_pos = e.next_pos, q.tlen = e.tlen;
    q.flag = e.flag, q.mapq = e.mapq;
    q.pos = A.dump_pos[r];
    const int64_t d = (int64_t)A.rec[4 * r];
    const int L = A.dump_len[r];
    q.L = d + L <= A.n_dump ? L : 0;
    q.sq = A.dump_seq + d;
    q.ql = A.dump_qual + d;
    const uint32_t t = A.dump_tags[r];
    q.rd = t & 1u;
    q.conv = (t & 2u) != 0;
    q.pre = (t & 6u) != 0;
    const int app = (t & 8u) != 0;
    // RD of a record converted here takes 1 off the last op of [1M] + ops, or drops it at length <= 1
    const bool trim = q.conv && q.rd;
    const uint32_t last = q.n ? q.cg[q.n - 1] >> 4 : 1u;
    const int drop = trim && last <= 1u;
    q.dec = trim && last > 1u;
    q.body = q.pre + q.n - drop;
    q.nc = q.body + app;
    q.o_cig = 36 + q.nl + 1;
    q.o_seq = q.o_cig + 4 * q.nc;
    q.o_qual = q.o_seq + (q.L + 1) / 2;
    q.o_aux = q.o_qual + q.L;
    q.o_tags = q.o_aux + q.al;
    q.size = q.ok ? q.o_tags + (q.conv ? 8 : 0) : 0;
    return q;
}

// op j of the record's new cigar (0 <= j < nc)
BSDC_HD uint32_t tr_op(const TrRec &q, int j) {
    if (j >= q.body || j < q.pre) return kOp1M;
    const uint32_t op = q.cg[j - q.pre];
    return q.dec && j == q.body - 1 ? op - kOp1M : op;
}
// the reference bases an op consumes: M D N = X
BSDC_HD int64_t tr_op_ref(uint32_t op) {
    const uint32_t k = op & 15u;
    return (k == 0 || k == 2 || k == 3 || k == 7 || k == 8) ? (int64_t)(op >> 4) : 0;
}
// this lane's share of the new cigar's reference length (lanes lane, lane + nl, ..)
BSDC_HD int64_t tr_reflen_part(const TrRec &q, int lane, int nlanes) {
    int64_t s = 0;
    for (int j = lane; j < q.nc; j += nlanes) s += tr_op_ref(tr_op(q, j));
    return s;
}
BSDC_HD uint32_t tr_bin(const TrRec &q, int64_t reflen) {
    return tr_reg2bin((int64_t)q.pos, (int64_t)q.pos + (reflen > 0 ? reflen : 1));
}

// dword w of the record's first 36 bytes
BSDC_HD uint32_t tr_fixed(const TrRec &q, uint32_t bin, int w) {
    switch (w) {
    case 0: return (uint32_t)(q.size - 4);
    case 1: return (uint32_t)q.ref_id;
    case 2: return (uint32_t)q.pos;
    case 3: return (uint32_t)(q.nl + 1) | q.mapq << 8 | bin << 16;
    case 4: return (uint32_t)q.nc | q.flag << 16;
    case 5: return (uint32_t)q.L;
    case 6: return (uint32_t)q.next_ref_id;
    case 7: return (uint32_t)q.next_pos;
    default: return (uint32_t)q.tlen;
    }
}

// byte i of the record (0 outside it)
BSDC_HD uint32_t tr_byte(const TrRec &q, uint32_t bin, int i) {
    if (i < 0 || i >= q.size) return 0;
    if (i < 36) return (tr_fixed(q, bin, i >> 2) >> (8 * (i & 3))) & 0xffu;
    if (i < q.o_cig) return i - 36 < q.nl ? (uint32_t)q.nm[i - 36] : 0u;
    if (i < q.o_seq) return (tr_op(q, (i - q.o_cig) >> 2) >> (8 * ((i - q.o_cig) & 3))) & 0xffu;
    if (i < q.o_qual) {
        const int j = 2 * (i - q.o_seq);
        return ((uint32_t)q.sq[j] & 15u) << 4 | (j + 1 < q.L ? (uint32_t)q.sq[j + 1] & 15u : 0u);  // (the pad nibble of an odd length is 0)
    }
    if (i < q.o_aux) return q.ql[i - q.o_qual];
    if (i < q.o_tags) return q.ax[i - q.o_aux];
    const int t = i - q.o_tags;  // RD:C:rd LA:C:1
    return t == 0 ? 'R' : t == 1 ? 'D' : t == 3 ? q.rd : t == 4 ? 'L' : t == 5 ? 'A' : t == 7 ? 1u : 'C';
}

// bytes i0 .. i0 + 3 of the record as one little-endian dword (bytes outside the record: 0)
BSDC_HD uint32_t tr_dword(const TrArgs &A, const TrRec &q, uint32_t bin, int i0) {
    if (i0 >= q.o_qual && i0 + 4 <= q.o_aux) {
        const uint8_t *a = q.ql + (i0 - q.o_qual);
        if (can4(A.dump_qual, A.n_dump, a)) return load4(a);
    } else if (i0 >= q.o_seq && i0 + 4 <= q.o_seq + q.L / 2) {  // (whole bytes only: eight codes inside the read)
        const uint8_t *a = q.sq + 2 * (i0 - q.o_seq);
        if (can4(A.dump_seq, A.n_dump, a) && can4(A.dump_seq, A.n_dump, a + 4))
            return tr_pack4(load4(a)) | tr_pack4(load4(a + 4)) << 16;
    } else if (i0 >= q.o_aux && i0 + 4 <= q.o_tags) {
        const uint8_t *a = q.ax + (i0 - q.o_aux);
        if (can4(A.aux, A.aux_bytes, a)) return load4(a);
    }
    uint32_t x = 0;
    for (int b = 0; b < 4; b++) x |= tr_byte(q, bin, i0 + b) << (8 * b);
    return x;
}

// the record's bytes at dst + o, this lane's dwords (lanes lane, lane + nlanes, ..)
BSDC_HD void tr_store(const TrArgs &A, const TrRec &q, uint32_t bin, int64_t o, int lane, int nlanes) {
    store_record(A.dst, o, q.size, A.cap, lane, nlanes, [&](int i0) { return tr_dword(A, q, bin, i0); });
}

thread_local std::string g_tr_err;

int32_t tr_fail(const std::string &m) {
    g_tr_err = m;
    return BSDC_EINVAL;
}

int64_t tr_bound(int64_t n_rec, int64_t name_bytes, int64_t n_ops, int64_t aux_bytes, int64_t n_dump) {
    if (n_rec < 0 || name_bytes < 0 || n_ops < 0 || aux_bytes < 0 || n_dump < 0) return -1;
    // a record: block_size, 32 fixed bytes, the name's NUL, two added cigar ops, the pad nibble's byte,
    // RD and LA; the names, the ops and the aux as they are; SEQ and QUAL of the records' dump
    // slots, which do not overlap: at most n_dump bases in all
    return n_rec * (36 + 1 + 8 + 1 + 8) + name_bytes + 4 * n_ops + aux_bytes + n_dump + n_dump / 2;
}

// the arguments, as the launcher and the twin both refuse them (tab: a host copy); fills A
int32_t tr_check(const char *who, const bsdc_consensus *out, const uint32_t *rec, int64_t n_rec, int64_t n_dump,
                 const bsdc_toolrec_rec *dev_tab, const bsdc_toolrec_rec *tab, const uint8_t *names, int64_t name_bytes,
                 const uint32_t *cigar, int64_t n_ops, const uint8_t *aux, int64_t aux_bytes, int64_t *off, uint8_t *dst,
                 int64_t cap, TrArgs *A) {
    const std::string w(who);
    if (!out) return tr_fail(w + ": out is null");
    if (!out->dump_pos) return tr_fail(w + ": dump_pos is null (the stage dump of a BSDC_MODE_DUMP run)");
    if (!out->dump_len) return tr_fail(w + ": dump_len is null (the stage dump of a BSDC_MODE_DUMP run)");
    if (!out->dump_tags) return tr_fail(w + ": dump_tags is null (the stage dump of a BSDC_MODE_DUMP run)");
    if (!out->dump_seq) return tr_fail(w + ": dump_seq is null (the stage dump of a BSDC_MODE_DUMP run)");
    if (!out->dump_qual) return tr_fail(w + ": dump_qual is null (the stage dump of a BSDC_MODE_DUMP run)");
    if (n_rec < 0 || n_rec > (int64_t)1 << 30) return tr_fail(w + ": n_rec is negative or beyond 2^30");
    if (n_dump < 0) return tr_fail(w + ": n_dump is negative");
    if (name_bytes < 0) return tr_fail(w + ": name_bytes is negative");
    if (n_ops < 0) return tr_fail(w + ": n_ops is negative");
    if (aux_bytes < 0) return tr_fail(w + ": aux_bytes is negative");
    if (!rec) return tr_fail(w + ": rec is null");
    if (!dev_tab || !tab) return tr_fail(w + ": tab is null");
    if (!names) return tr_fail(w + ": names is null");
    if (!cigar) return tr_fail(w + ": cigar is null");
    if (!aux) return tr_fail(w + ": aux is null");
    if (!off) return tr_fail(w + ": off is null");
    if (!dst) return tr_fail(w + ": dst is null");
    if (cap < tr_bound(n_rec, name_bytes, n_ops, aux_bytes, n_dump))
        return tr_fail(w + ": cap " + std::to_string(cap) + " is below bsdc_toolrec_bytes_bound " +
                       std::to_string(tr_bound(n_rec, name_bytes, n_ops, aux_bytes, n_dump)));
    if (((uintptr_t)out->dump_seq & 3u) || ((uintptr_t)out->dump_qual & 3u) || ((uintptr_t)aux & 3u) ||
        ((uintptr_t)cigar & 3u) || ((uintptr_t)rec & 3u) || ((uintptr_t)out->dump_pos & 3u) || ((uintptr_t)out->dump_len & 1u))
        return tr_fail(w + ": the dump, rec, cigar and aux buffers must be 4-byte aligned");
    if (((uintptr_t)off & 7u) || ((uintptr_t)dev_tab & 7u)) return tr_fail(w + ": off and tab must be 8-byte aligned");
    for (int64_t r = 0; r < n_rec; r++) {
        const bsdc_toolrec_rec &e = tab[r];
        const char *bad = nullptr;  // (the message is made for a refused record only: this loop is on the launch path)
        if (e.name_len < 1 || e.name_len > kTrMaxName) bad = "name_len outside 1..254";
        else if (e.name_off < 0 || e.name_off + e.name_len > name_bytes) bad = "its name leaves names";
        else if (e.n_cig < 0 || e.n_cig > kTrMaxCig) bad = "n_cig outside 0..65533";
        else if (e.cig_off < 0 || e.cig_off + e.n_cig > n_ops) bad = "its ops leave cigar";
        else if (e.aux_len < 0 || e.aux_len > kTrMaxAux) bad = "aux_len outside 0..2^24";
        else if (e.aux_off < 0 || e.aux_off + e.aux_len > aux_bytes) bad = "its aux bytes leave aux";
        if (bad) return tr_fail(w + ": record " + std::to_string(r) + ": " + bad);
    }
    A->dump_pos = out->dump_pos, A->dump_len = out->dump_len, A->dump_tags = out->dump_tags;
    A->dump_seq = out->dump_seq, A->dump_qual = out->dump_qual;
    A->rec = rec, A->tab = dev_tab, A->names = names, A->cigar = cigar, A->aux = aux;
    A->n_fam = n_rec, A->n_dump = n_dump, A->name_bytes = name_bytes, A->n_ops = n_ops, A->aux_bytes = aux_bytes;
    A->off = off, A->dst = dst, A->cap = cap;
    A->bsum = nullptr, A->stat = nullptr, A->groups = 0;
    return 0;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kT) void k_toolrec_sizes(TrArgs A) {
    const int64_t r = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    if (r >= A.n_fam) return;
    const int lane = threadIdx.x & 63;
    const TrRec q = tr_rec(A, r);
    const int64_t reflen = wave_sum(tr_reflen_part(q, lane, 64));
    if (lane < kTrStat) A.stat[r * kTrStat + lane] = lane == 0 ? (uint32_t)q.size : tr_bin(q, reflen);
}

__global__ __launch_bounds__(kT) void k_toolrec_write(TrArgs A) {
    const int64_t r = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    if (r >= A.n_fam) return;
    const TrRec q = tr_rec(A, r);
    tr_store(A, q, A.stat[r * kTrStat + 1], A.off[r], threadIdx.x & 63, 64);
}

int64_t tr_groups(int64_t n_rec) { return (n_rec + kFamPerGroup - 1) / kFamPerGroup; }
#endif

}  // namespace

extern "C" {

const char *bsdc_toolrec_last_error(void) { return g_tr_err.c_str(); }

int64_t bsdc_toolrec_bytes_bound(int64_t n_rec, int64_t name_bytes, int64_t n_ops, int64_t aux_bytes, int64_t n_dump) {
    return tr_bound(n_rec, name_bytes, n_ops, aux_bytes, n_dump);
}

int32_t bsdc_toolrec_host(const bsdc_consensus *out, const uint32_t *rec, int64_t n_rec, int64_t n_dump,
                          const bsdc_toolrec_rec *tab, const uint8_t *names, int64_t name_bytes, const uint32_t *cigar,
                          int64_t n_ops, const uint8_t *aux, int64_t aux_bytes, int64_t *off, uint8_t *dst, int64_t cap) {
    TrArgs A;
    if (const int32_t rc = tr_check("bsdc_toolrec_host", out, rec, n_rec, n_dump, tab, tab, names, name_bytes, cigar, n_ops,
                                    aux, aux_bytes, off, dst, cap, &A))
        return rc;
    for (int64_t r = 0; r < n_rec; r++)  // (host pointers: the dump's own table is checked here as well)
        if ((int64_t)rec[4 * r] + out->dump_len[r] > n_dump)
            return tr_fail("bsdc_toolrec_host: record " + std::to_string(r) + ": its dump slot leaves the dump (n_dump)");
    int64_t o = 0;
    for (int64_t r = 0; r < n_rec; r++) {
        const TrRec q = tr_rec(A, r);
        off[r] = o;
        tr_store(A, q, tr_bin(q, tr_reflen_part(q, 0, 1)), o, 0, 1);
        o += q.size;
    }
    off[n_rec] = o;
    return 0;
}

#ifdef __HIPCC__
int64_t bsdc_toolrec_tmp_bytes(int64_t n_rec) {
    if (n_rec < 0) return -1;
    return (tr_groups(n_rec) + 1) * (int64_t)sizeof(int64_t) + n_rec * kTrStat * (int64_t)sizeof(uint32_t) + 8;
}

int32_t bsdc_toolrec_format(const bsdc_consensus *out, const uint32_t *rec, int64_t n_rec, int64_t n_dump,
                            const bsdc_toolrec_rec *tab, const bsdc_toolrec_rec *tab_host, const uint8_t *names,
                            int64_t name_bytes, const uint32_t *cigar, int64_t n_ops, const uint8_t *aux, int64_t aux_bytes,
                            int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream) {
    TrArgs A;
    if (const int32_t rc = tr_check("bsdc_toolrec_format", out, rec, n_rec, n_dump, tab, tab_host, names, name_bytes, cigar,
                                    n_ops, aux, aux_bytes, off, dst, cap, &A))
        return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return tr_fail("bsdc_toolrec_format: tmp is null or not 8-byte aligned");
    A.groups = tr_groups(n_rec);
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    A.stat = reinterpret_cast<uint32_t *>(tmp + (A.groups + 1) * sizeof(int64_t));
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)((n_rec + kT / 64 - 1) / (kT / 64));
    if (wgs) hipLaunchKernelGGL(k_toolrec_sizes, dim3(wgs), dim3(kT), 0, st, A);
    launch_scan<1>(A, st);
    if (wgs) hipLaunchKernelGGL(k_toolrec_write, dim3(wgs), dim3(kT), 0, st, A);
    if (hipGetLastError() != hipSuccess) {
        g_tr_err = "bsdc_toolrec_format: a kernel launch failed";
        return BSDC_EDEVICE;
    }
    return 0;
}
#endif

}  // extern "C"
