// cli group on the GPU (gfx950): paired-UMI molecule ids for the templates of a tagged BAM -- what
// `fgbio GroupReadsByUmi -s Paired` leaves, the input of cli molecular (rules in DESIGN.md section
// 3.12, these kernels in 8.13; declarations and the rule text in include/bsdc.h).  Two pieces, each
// with a host twin made of the same per-node and per-record functions:
//
// bsdc_group_assign, over templates in read-name order (k0 / k1: the lower / higher end's packed
// position key, umi: the packed canonical UMI, strand: 0 top, 1 bottom):
//  1. the templates sorted by (k0, k1, umi, name order): three stable sorts by bsdc_zip_sort (the
//     radix passes of bsdc_zipper.hip, called, not copied), the next key word gathered between them;
//  2. k_grp_flags marks where a position group / a node (one canonical UMI of a group) starts, the
//     offset scan of bsdc_devtext.h numbers them, k_grp_bounds notes their first templates / nodes;
//  3. the nodes sorted by (group, n - count) (bsdc_zip_sort again: stable, so equal counts keep
//     their UMI order): rule 4's order, k_grp_nodes gathers their UMIs and counts in that order;
//  4. k_group_small: a wavefront per group of at most 64 nodes, a lane per node.  The FIFO of rule 5
//     is a register a lane (its place in the FIFO): the parent of a round is the lane whose place
//     is `head` (one ballot), its UMI and count are broadcast, every unassigned lane tests itself,
//     a ballot and a prefix popcount give the joiners their places in node order.  Groups of more
//     nodes are listed (an atomic counter; their order does not matter) for
//     k_group_large: a workgroup of 1024 per group, thread t owning a contiguous run of nodes, so
//     that thread order is node order: a round counts each thread's joiners, scans the counts over
//     the workgroup (wave scans + the waves' totals) and appends them to the FIFO in that order.
//     UMIs, counts, FIFO and `assigned` bytes lie in LDS up to kGrpLdsNodes nodes, else the FIFO
//     and the bytes lie in the caller's scratch and UMIs and counts are read where step 3 left them;
//  5. roots flagged and scanned -> molecule ids; k_grp_number gives every template its id and /A or
//     /B (against the root node's first template) and the key id << 1 | B, which one more stable
//     sort from name order turns into rule 7's output order.
//
// bsdc_group_format: one wavefront per output record (R1 then R2 of each template in output
// order): k_group_sizes, the offset scan, k_group_write -- the record's bytes before the aux, the
// aux walked by type (bsdc_auxwalk.h) with the assign tag left out, and the tag with the id in
// decimal appended; a lane writes the bytes it owns.  No byte at or past `cap` is written; a table
// entry that leaves `rec`, or an order entry >= n, makes a record of size 0.  The launcher refuses
// bad table entries and malformed aux blocks from the host copies first; `order` is a device array
// that it does not read (the host twin, which can, refuses an entry >= n).
// Limits: bsdc_group_assign takes n <= 2^30 templates (bsdc_zip_sort's limit), bsdc_group_format
// n <= 2^29 (its 2n records are the offset scan's items).
// Built without hipcc this file holds the twins alone.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/bsdc.h"
#include "bsdc_auxwalk.h"
#include "bsdc_devtext.h"

namespace {

using namespace bsdc_devtext;

constexpr int kGrpSmallNodes = 64;            // k_group_small: a lane a node
constexpr int kGrpLargeThreads = 1024;
constexpr int kGrpNodeBytes = 8 + 4 + 4 + 1;  // LDS per node: UMI, count, FIFO entry, assigned
constexpr int kGrpLdsBytes = 128 * 1024;      // of the CU's 160 KB
constexpr int kGrpLdsNodes = kGrpLdsBytes / kGrpNodeBytes;
constexpr int kGrpTagMax = 3 + 10 + 2 + 1;    // MIZ, ten digits, /A, NUL

// ---- rule 5 ----

// differing bases of two packed canonical UMIs (two bits a base, both halves)
BSDC_HD uint32_t grp_hamming(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    return (uint32_t)__builtin_popcountll((x | x >> 1) & 0x5555555555555555ull);
}
// node c (count cc) joins the molecule of parent p (count pc)
BSDC_HD bool grp_joins(uint64_t pu, uint32_t pc, uint64_t cu, uint32_t cc, int edits) {
    return cc <= pc / 2 + 1 && grp_hamming(pu, cu) <= (uint32_t)edits;
}

// the key bounds bsdc_zip_sort skips passes by, for keys <= m (or whose OR is m)
void grp_sort_bounds(uint64_t m, int32_t *max_ref, int32_t *max_pos) {
    const uint32_t hi = (uint32_t)(m >> 32), lo = (uint32_t)m;
    *max_ref = hi > 0x7fffffffu ? 0x7fffffff : (int32_t)hi;
    *max_pos = (lo >> 1) > 0x7ffffffeu ? 0x7ffffffe : (int32_t)(lo >> 1);
}

thread_local std::string g_grp_err;

int32_t grp_fail(const std::string &m) {
    g_grp_err = m;
    return BSDC_EINVAL;
}

int32_t ga_check(const char *who, const uint64_t *k0, const uint64_t *k1, const uint64_t *umi, const uint8_t *strand, int64_t n,
                 int32_t edits, const uint64_t *kmax, const uint32_t *mol, const uint8_t *ab, const uint32_t *order,
                 const int64_t *stats) {
    const std::string w(who);
    if (n < 0 || n > (int64_t)1 << 30) return grp_fail(w + ": n is negative or beyond 2^30");
    if (edits < 0 || edits > 3) return grp_fail(w + ": edits is outside 0..3");
    if (!k0 || !k1 || !umi || !strand || !kmax || !mol || !ab || !order || !stats) return grp_fail(w + ": a null pointer");
    if (((uintptr_t)k0 & 7u) || ((uintptr_t)k1 & 7u) || ((uintptr_t)umi & 7u) || ((uintptr_t)mol & 3u) || ((uintptr_t)order & 3u))
        return grp_fail(w + ": the keys must be 8-byte, mol and order 4-byte aligned");
    return 0;
}

// ---- the records ----

struct GwArgs {
    const uint32_t *order;  // [n_tpl] the template of output place k
    const uint32_t *mol;    // [n_tpl]
    const uint8_t *ab;      // [n_tpl]
    const bsdc_group_rec *tab;  // [2 n_tpl]: R1, R2 of template t at 2t, 2t + 1
    const uint8_t *rec;
    int64_t rec_bytes, n_tpl;
    uint8_t tag0, tag1;
    int64_t n_fam;  // 2 n_tpl: the output records (the scan's name for its items)
    int64_t *off;
    uint8_t *dst;
    int64_t cap;
    int64_t *bsum;
    uint32_t *stat;  // [n_fam] sizes
    int64_t groups;
};
BSDC_HD int64_t scan_bytes(const GwArgs &A, int64_t r, int) { return (int64_t)A.stat[r]; }
BSDC_HD int64_t *scan_off(const GwArgs &A, int) { return A.off; }

BSDC_HD int grp_digits(uint32_t v) {
    int d = 1;
    while (v >= 10) v /= 10, d++;
    return d;
}
// byte i of the tag of molecule `mol`, strand b: NN Z <decimal> / A|B NUL (nd: the id's digits)
BSDC_HD uint8_t grp_tag_byte(const GwArgs &A, uint32_t mol, int b, int nd, int i) {
    if (i == 0) return A.tag0;
    if (i == 1) return A.tag1;
    if (i == 2) return 'Z';
    if (i < 3 + nd) {
        uint32_t v = mol;
        for (int k = 3 + nd - 1; k > i; k--) v /= 10;
        return (uint8_t)('0' + v % 10);
    }
    if (i == 3 + nd) return '/';
    if (i == 4 + nd) return b ? 'B' : 'A';
    return 0;
}

// One output record.  Everything here is the same in every lane of its wavefront.
struct GwRec {
    const uint8_t *r;  // the input record (its block_size field)
    int64_t rn, ra;    // its bytes, its aux start (0: no record)
    uint32_t mol;
    int b;
};

BSDC_HD GwRec gw_rec(const GwArgs &A, int64_t k) {
    GwRec q;
    const uint32_t t = A.order[k >> 1];
    const bool in = (int64_t)t < A.n_tpl;
    bsdc_group_rec e;
    e.off = 0, e.len = 0, e.aux = 0;
    if (in) e = A.tab[2 * (int64_t)t + (k & 1)];
    const bool ok = in && e.len >= 36 && e.aux >= 36 && e.aux <= e.len && e.off >= 0 && e.off + e.len <= A.rec_bytes;
    q.r = A.rec + (ok ? e.off : 0);
    q.rn = ok ? e.len : 0, q.ra = ok ? e.aux : 0;
    q.mol = ok ? A.mol[t] : 0, q.b = ok ? A.ab[t] & 1 : 0;
    return q;
}

BSDC_HD void gw_put(const GwArgs &A, int64_t p, uint8_t v) {
    if (p >= 0 && p < A.cap) A.dst[p] = v;
}

// The record at dst + o (WRITE) -> its size.  `size`: what the size pass gave (the block_size field).
template <bool WRITE>
BSDC_HD int64_t gw_emit(const GwArgs &A, const GwRec &q, uint32_t size, int64_t o, int lane, int nlanes) {
    if (q.rn == 0) return 0;
    int64_t w = q.ra;
    if (WRITE)
        for (int64_t i = lane; i < q.ra; i += nlanes) gw_put(A, o + i, i < 4 ? (uint8_t)((size - 4) >> (8 * i)) : q.r[i]);
    const uint8_t *ax = q.r + q.ra;
    const int64_t an = q.rn - q.ra;
    for (int64_t i = 0; i < an;) {
        const int64_t j = zp_tag_end(ax, i, an);
        if (j < 0) break;
        if (!(ax[i] == A.tag0 && ax[i + 1] == A.tag1)) {
            if (WRITE)
                for (int64_t b = lane; b < j - i; b += nlanes) gw_put(A, o + w + b, ax[i + b]);
            w += j - i;
        }
        i = j;
    }
    const int nd = grp_digits(q.mol), tn = 3 + nd + 3;
    if (WRITE)
        for (int i = lane; i < tn; i += nlanes) gw_put(A, o + w + i, grp_tag_byte(A, q.mol, q.b, nd, i));
    return w + tn;
}

int64_t gw_bound(const bsdc_group_rec *tab, int64_t n_rec) {
    if (n_rec < 0 || (n_rec && !tab)) return -1;
    int64_t s = 0;
    for (int64_t k = 0; k < n_rec; k++) {
        if (tab[k].len < 0) return -1;
        s += (int64_t)tab[k].len + kGrpTagMax;
    }
    return s;
}

int32_t gw_check(const char *who, const uint32_t *order, const uint32_t *mol, const uint8_t *ab, int64_t n,
                 const bsdc_group_rec *dev_tab, const bsdc_group_rec *tab, const uint8_t *rec, const uint8_t *rec_host,
                 int64_t rec_bytes, const char *tag, int64_t *off, uint8_t *dst, int64_t cap, GwArgs *A) {
    const std::string w(who);
    if (n < 0 || n > (int64_t)1 << 29) return grp_fail(w + ": n is negative or beyond 2^29");
    if (rec_bytes < 0) return grp_fail(w + ": a negative byte count");
    if (!order || !mol || !ab || !dev_tab || !tab || !rec || !rec_host || !tag || !off || !dst) return grp_fail(w + ": a null pointer");
    if (!tag[0] || !tag[1] || tag[2]) return grp_fail(w + ": the tag name has two letters");
    if (((uintptr_t)order & 3u) || ((uintptr_t)mol & 3u) || ((uintptr_t)off & 7u) || ((uintptr_t)dev_tab & 7u))
        return grp_fail(w + ": order and mol must be 4-byte, off and tab 8-byte aligned");
    for (int64_t k = 0; k < 2 * n; k++) {
        const bsdc_group_rec &e = tab[k];
        const char *bad = nullptr;
        if (e.len < 36 || e.aux < 36 || e.aux > e.len) bad = "len or aux outside the record";
        else if (e.off < 0 || e.off + e.len > rec_bytes) bad = "its bytes leave rec";
        if (bad) return grp_fail(w + ": record " + std::to_string(k) + ": " + bad);
        const std::string m = zp_aux_error(rec_host + e.off + e.aux, e.len - e.aux);
        if (!m.empty()) return grp_fail(w + ": record " + std::to_string(k) + " (read " + zp_name(rec_host + e.off, e.len) + "): " + m);
    }
    const int64_t need = gw_bound(tab, 2 * n);
    if (need < 0 || cap < need) return grp_fail(w + ": cap " + std::to_string(cap) + " is below bsdc_group_bytes_bound " + std::to_string(need));
    A->order = order, A->mol = mol, A->ab = ab, A->tab = dev_tab, A->rec = rec, A->rec_bytes = rec_bytes, A->n_tpl = n;
    A->tag0 = (uint8_t)tag[0], A->tag1 = (uint8_t)tag[1];
    A->n_fam = 2 * n, A->off = off, A->dst = dst, A->cap = cap;
    A->bsum = nullptr, A->stat = nullptr, A->groups = 0;
    return 0;
}

#ifdef __HIPCC__
// ---- the device pipeline ----

struct GaArgs {
    const uint64_t *k0, *k1, *umi;  // [n] templates in name order
    const uint8_t *strand;
    int64_t n;
    int edits;
    uint64_t *keys;  // [n] the sort's keys (the template sorts, then id << 1 | B)
    uint32_t *idx;   // [n] the templates in (k0, k1, umi, name) order
    uint8_t *flag;   // [2][n] a group / a node starts here
    int64_t *foff;   // [2][n + 1] their exclusive scans: totals at [n]
    uint32_t *nstart;  // [nodes + 1] a node's first sorted template (nodes in (group, umi) order)
    uint32_t *gstart;  // [groups + 1] a group's first node
    uint64_t *nkeys;   // [nodes]
    uint32_t *nidx;    // [nodes] the nodes in rule 4's order
    uint64_t *s_umi;   // [nodes] in rule 4's order, as are:
    uint32_t *s_cnt, *root, *fifo;
    uint8_t *asg, *isroot;
    uint32_t *npos;   // [nodes] a node's place in rule 4's order
    int64_t *roff;    // [nodes + 1] roots before a node: the molecule ids
    uint32_t *large;  // [groups] groups of more than kGrpSmallNodes nodes
    uint32_t *counters;  // [2] their number, the most nodes of a group
    uint32_t *mol, *order;
    uint8_t *ab;
    int64_t n_nodes, n_groups;
};

// the offset scan's view: D flag rows of n_fam items
struct GsArgs {
    const uint8_t *f;  // [D][n_fam]
    int64_t *o;        // [D][n_fam + 1]
    int64_t n_fam, groups;
    int64_t *bsum;
};
BSDC_HD int64_t scan_bytes(const GsArgs &A, int64_t i, int d) { return (int64_t)A.f[d * A.n_fam + i]; }
BSDC_HD int64_t *scan_off(const GsArgs &A, int d) { return A.o + d * (A.n_fam + 1); }

__device__ __forceinline__ int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(kT) void k_grp_iota(uint32_t *idx, int64_t n) {
    const int64_t i = gid();
    if (i < n) idx[i] = (uint32_t)i;
}
__global__ __launch_bounds__(kT) void k_grp_gather(uint64_t *keys, const uint64_t *src, const uint32_t *idx, int64_t n) {
    const int64_t i = gid();
    if (i < n) {
        const uint32_t t = idx[i];
        keys[i] = (int64_t)t < n ? src[t] : 0;
    }
}
__global__ __launch_bounds__(kT) void k_grp_flags(GaArgs A) {
    const int64_t i = gid();
    if (i >= A.n) return;
    bool g = true, u = true;
    if (i > 0) {
        const uint32_t t = A.idx[i], p = A.idx[i - 1];
        g = A.k0[t] != A.k0[p] || A.k1[t] != A.k1[p];
        u = g || A.umi[t] != A.umi[p];
    }
    A.flag[i] = g, A.flag[A.n + i] = u;
}
__global__ __launch_bounds__(kT) void k_grp_bounds(GaArgs A) {
    const int64_t i = gid();
    if (i >= A.n) return;
    const int64_t *goff = A.foff, *noff = A.foff + A.n + 1;
    if (A.flag[A.n + i]) {
        const int64_t u = noff[i];
        if (u <= A.n) A.nstart[u] = (uint32_t)i;
        if (A.flag[i] && goff[i] <= A.n) A.gstart[goff[i]] = (uint32_t)u;
    }
    if (i == A.n - 1) {
        if (noff[A.n] <= A.n) A.nstart[noff[A.n]] = (uint32_t)A.n;
        if (goff[A.n] <= A.n) A.gstart[goff[A.n]] = (uint32_t)noff[A.n];
    }
}
__global__ __launch_bounds__(kT) void k_grp_nodekeys(GaArgs A) {
    const int64_t u = gid();
    if (u >= A.n_nodes) return;
    const int64_t i = A.nstart[u];
    const uint32_t cnt = A.nstart[u + 1] - A.nstart[u];
    const int64_t g = i < A.n ? A.foff[i] + A.flag[i] - 1 : 0;
    A.nkeys[u] = (uint64_t)g << 32 | (uint64_t)((uint32_t)A.n - cnt);
    A.nidx[u] = (uint32_t)u;
}
__global__ __launch_bounds__(kT) void k_grp_nodes(GaArgs A) {
    const int64_t j = gid();
    if (j >= A.n_nodes) return;
    const uint32_t u = A.nidx[j];
    if ((int64_t)u >= A.n_nodes) return;
    const uint32_t i = A.nstart[u];
    A.s_umi[j] = i < A.n ? A.umi[A.idx[i]] : 0;
    A.s_cnt[j] = A.nstart[u + 1] - i;
    A.npos[u] = (uint32_t)j;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(kT) void k_group_small(GaArgs A) {
    const int64_t g = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= A.n_groups) return;
    const int lane = threadIdx.x & 63;
    const uint32_t nb = A.gstart[g], m = A.gstart[g + 1] - nb;
    if (m == 1) {
        if (lane == 0) A.root[nb] = nb;
        return;
    }
    if (lane == 0) atomicMax(&A.counters[1], m);
    if (m > (uint32_t)kGrpSmallNodes) {
        if (lane == 0) {
            const uint32_t k = atomicAdd(&A.counters[0], 1u);
            if ((int64_t)k < A.n_groups) A.large[k] = (uint32_t)g;
        }
        return;
    }
    const bool valid = (uint32_t)lane < m;
    const uint64_t umi = valid ? A.s_umi[nb + lane] : 0;
    const uint32_t cnt = valid ? A.s_cnt[nb + lane] : 0;
    uint64_t un = m == 64 ? ~0ull : (1ull << m) - 1ull;  // the unassigned nodes
    uint32_t myroot = 0;
    int mypos = -1, head = 0, tail = 0;  // mypos: this node's place in the FIFO
    while (un) {
        const int r = __ffsll((long long)un) - 1;
        un &= ~(1ull << r);
        if (lane == r) myroot = (uint32_t)r, mypos = tail;
        tail++;
        while (head < tail && un) {
            const int p = __ffsll((long long)__ballot(mypos == head)) - 1;
            head++;
            const uint64_t pu = shfl64(umi, p);
            const uint32_t pc = (uint32_t)__shfl((int)cnt, p, 64);
            const bool j = ((un >> lane) & 1ull) && grp_joins(pu, pc, umi, cnt, A.edits);
            const uint64_t b = __ballot(j);
            if (j) myroot = (uint32_t)r, mypos = tail + __popcll(b & ((1ull << lane) - 1ull));
            un &= ~b;
            tail += __popcll(b);
        }
        head = tail;
    }
    if (valid) A.root[nb + lane] = nb + myroot;
}

// exclusive scan of one value per thread over the 1024 threads (ws: 16 words); *total = the sum
__device__ __forceinline__ uint32_t grp_block_scan(uint32_t v, uint32_t *ws, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += x;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kGrpLargeThreads / 64; w++) {
        const uint32_t x = ws[w];
        if (w < wave) before += x;
        all += x;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kGrpLargeThreads) void k_group_large(GaArgs A, int lds_nodes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t ws[kGrpLargeThreads / 64];
    const uint32_t g = A.large[blockIdx.x];
    if ((int64_t)g >= A.n_groups) return;
    const uint32_t nb = A.gstart[g], m = A.gstart[g + 1] - nb;
    const uint32_t t = threadIdx.x;
    const uint64_t *umi = A.s_umi + nb;
    const uint32_t *cnt = A.s_cnt + nb;
    uint32_t *fifo = A.fifo + nb;
    uint8_t *asg = A.asg + nb;
    if (m <= (uint32_t)lds_nodes) {  // (the same for the whole workgroup)
        uint64_t *lu = reinterpret_cast<uint64_t *>(smem);
        uint32_t *lc = reinterpret_cast<uint32_t *>(smem + 8 * (size_t)m);
        fifo = reinterpret_cast<uint32_t *>(smem + 12 * (size_t)m);
        asg = smem + 16 * (size_t)m;
        for (uint32_t i = t; i < m; i += kGrpLargeThreads) lu[i] = umi[i], lc[i] = cnt[i];
        umi = lu, cnt = lc;
    }
    for (uint32_t i = t; i < m; i += kGrpLargeThreads) asg[i] = 0;
    __syncthreads();
    const uint32_t per = (m + kGrpLargeThreads - 1) / kGrpLargeThreads;
    const uint32_t c0 = t * per < m ? t * per : m, c1 = c0 + per < m ? c0 + per : m;  // this thread's nodes
    uint32_t head = 0, tail = 0, next = 0;
    for (;;) {
        while (next < m && asg[next]) next++;  // (every thread reads the same bytes)
        if (next >= m) break;
        const uint32_t r = next;
        __syncthreads();
        if (t == 0) asg[r] = 1, fifo[tail] = r, A.root[nb + r] = nb + r;
        tail++;
        __syncthreads();
        while (head < tail) {
            const uint32_t p = fifo[head++];
            const uint64_t pu = umi[p];
            const uint32_t pc = cnt[p];
            uint32_t k = 0;
            for (uint32_t c = c0; c < c1; c++) k += !asg[c] && grp_joins(pu, pc, umi[c], cnt[c], A.edits);
            uint32_t total;
            uint32_t o = tail + grp_block_scan(k, ws, &total);
            if (k)
                for (uint32_t c = c0; c < c1; c++)
                    if (!asg[c] && grp_joins(pu, pc, umi[c], cnt[c], A.edits)) {
                        asg[c] = 1;
                        if (o < m) fifo[o] = c;
                        o++;
                        A.root[nb + c] = nb + r;
                    }
            tail += total;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kT) void k_grp_isroot(GaArgs A) {
    const int64_t j = gid();
    if (j < A.n_nodes) A.isroot[j] = A.root[j] == (uint32_t)j;
}
__global__ __launch_bounds__(kT) void k_grp_number(GaArgs A) {
    const int64_t i = gid();
    if (i >= A.n) return;
    const uint32_t t = A.idx[i];
    const int64_t u = A.foff[A.n + 1 + i] + A.flag[A.n + i] - 1;
    if ((int64_t)t >= A.n || u < 0 || u >= A.n_nodes) return;
    const uint32_t r = A.root[A.npos[u]];
    if ((int64_t)r >= A.n_nodes) return;
    const int64_t id = A.roff[r];
    const uint32_t first = A.nstart[A.nidx[r]];  // the root node's first template: the lowest name
    const uint8_t b = first < A.n ? (A.strand[t] & 1) != (A.strand[A.idx[first]] & 1) : 0;
    A.mol[t] = (uint32_t)id, A.ab[t] = b;
    A.keys[t] = (uint64_t)id << 1 | b;
    A.order[t] = t;
}

__global__ __launch_bounds__(kT) void k_group_sizes(GwArgs A) {
    const int64_t k = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= A.n_fam) return;
    const GwRec q = gw_rec(A, k);
    const int64_t size = gw_emit<false>(A, q, 0, 0, 0, 64);
    if ((threadIdx.x & 63) == 0) A.stat[k] = (uint32_t)size;
}
__global__ __launch_bounds__(kT) void k_group_write(GwArgs A) {
    const int64_t k = (int64_t)blockIdx.x * (kT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= A.n_fam) return;
    const GwRec q = gw_rec(A, k);
    gw_emit<true>(A, q, A.stat[k], A.off[k], threadIdx.x & 63, 64);
}

int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }
int64_t scan_groups(int64_t n) { return (n + kFamPerGroup - 1) / kFamPerGroup; }
unsigned blocks(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

// tmp, carved: -> the bytes used (A == nullptr: the size alone)
int64_t ga_carve(int64_t n, uint8_t *tmp, GaArgs *A, uint8_t **sort_tmp, int64_t **bsum) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        uint8_t *p = tmp ? tmp + o : nullptr;
        o += up8(bytes);
        return p;
    };
    uint8_t *st = take(bsdc_zip_sort_tmp_bytes(n));
    int64_t *bs = (int64_t *)take(2 * (scan_groups(n) + 1) * 8);
    GaArgs B;
    B.keys = (uint64_t *)take(n * 8), B.idx = (uint32_t *)take(n * 4);
    B.flag = take(2 * n), B.foff = (int64_t *)take(2 * (n + 1) * 8);
    B.nstart = (uint32_t *)take((n + 1) * 4), B.gstart = (uint32_t *)take((n + 1) * 4);
    B.nkeys = (uint64_t *)take(n * 8), B.nidx = (uint32_t *)take(n * 4);
    B.s_umi = (uint64_t *)take(n * 8), B.s_cnt = (uint32_t *)take(n * 4), B.root = (uint32_t *)take(n * 4);
    B.fifo = (uint32_t *)take(n * 4), B.asg = take(n), B.isroot = take(n), B.npos = (uint32_t *)take(n * 4);
    B.roff = (int64_t *)take((n + 1) * 8), B.large = (uint32_t *)take(n * 4), B.counters = (uint32_t *)take(8);
    if (A) {
        A->keys = B.keys, A->idx = B.idx, A->flag = B.flag, A->foff = B.foff, A->nstart = B.nstart, A->gstart = B.gstart;
        A->nkeys = B.nkeys, A->nidx = B.nidx, A->s_umi = B.s_umi, A->s_cnt = B.s_cnt, A->root = B.root, A->fifo = B.fifo;
        A->asg = B.asg, A->isroot = B.isroot, A->npos = B.npos, A->roff = B.roff, A->large = B.large, A->counters = B.counters;
        *sort_tmp = st, *bsum = bs;
    }
    return o;
}
#endif

}  // namespace

extern "C" {

const char *bsdc_group_last_error(void) { return g_grp_err.c_str(); }

int32_t bsdc_group_lds_nodes(void) { return kGrpLdsNodes; }

int64_t bsdc_group_bytes_bound(const bsdc_group_rec *tab_host, int64_t n_rec) { return gw_bound(tab_host, n_rec); }

int32_t bsdc_group_assign_host(const uint64_t *k0, const uint64_t *k1, const uint64_t *umi, const uint8_t *strand, int64_t n,
                               int32_t edits, const uint64_t *kmax, uint32_t *mol, uint8_t *ab, uint32_t *order, int64_t *stats) {
    if (const int32_t rc = ga_check("bsdc_group_assign_host", k0, k1, umi, strand, n, edits, kmax, mol, ab, order, stats)) return rc;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return 0;
    const size_t N = (size_t)n;
    // 1. the templates by (k0, k1, umi, name order)
    std::vector<uint64_t> keys(N);
    std::vector<uint32_t> idx(N);
    for (size_t i = 0; i < N; i++) idx[i] = (uint32_t)i;
    const uint64_t *words[3] = {umi, k1, k0};
    for (int w = 0; w < 3; w++) {
        int32_t mr, mp;
        grp_sort_bounds(kmax[2 - w], &mr, &mp);
        for (size_t i = 0; i < N; i++) keys[i] = words[w][idx[i]];
        if (bsdc_zip_sort_host(keys.data(), idx.data(), n, mr, mp)) return grp_fail(std::string("bsdc_group_assign_host: ") + bsdc_zip_last_error());
    }
    // 2. groups and nodes
    std::vector<uint32_t> nstart, gstart, node_of(N);
    for (size_t i = 0; i < N; i++) {
        bool g = true, u = true;
        if (i > 0) {
            const uint32_t t = idx[i], p = idx[i - 1];
            g = k0[t] != k0[p] || k1[t] != k1[p];
            u = g || umi[t] != umi[p];
        }
        if (u) {
            if (g) gstart.push_back((uint32_t)nstart.size());
            nstart.push_back((uint32_t)i);
        }
        node_of[i] = (uint32_t)nstart.size() - 1;
    }
    const size_t nn = nstart.size(), ng = gstart.size();
    nstart.push_back((uint32_t)n), gstart.push_back((uint32_t)nn);
    // 3. rule 4's order
    std::vector<uint64_t> nkeys(nn);
    std::vector<uint32_t> nidx(nn), npos(nn), s_cnt(nn), root(nn);
    std::vector<uint64_t> s_umi(nn);
    for (size_t g = 0; g < ng; g++)
        for (uint32_t u = gstart[g]; u < gstart[g + 1]; u++)
            nkeys[u] = (uint64_t)g << 32 | (uint64_t)((uint32_t)n - (nstart[u + 1] - nstart[u])), nidx[u] = u;
    {
        int32_t mr, mp;
        grp_sort_bounds((uint64_t)(ng - 1) << 32 | (uint64_t)(uint32_t)n, &mr, &mp);
        if (bsdc_zip_sort_host(nkeys.data(), nidx.data(), (int64_t)nn, mr, mp)) return grp_fail(std::string("bsdc_group_assign_host: ") + bsdc_zip_last_error());
    }
    for (size_t j = 0; j < nn; j++) {
        const uint32_t u = nidx[j];
        s_umi[j] = umi[idx[nstart[u]]], s_cnt[j] = nstart[u + 1] - nstart[u], npos[u] = (uint32_t)j;
    }
    // 4. rule 5, group by group
    std::vector<uint32_t> fifo;
    std::vector<uint8_t> asg;
    uint32_t max_nodes = 0;
    for (size_t g = 0; g < ng; g++) {
        const uint32_t nb = gstart[g], m = gstart[g + 1] - nb;
        max_nodes = std::max(max_nodes, m);
        fifo.assign(m, 0), asg.assign(m, 0);
        uint32_t head = 0, tail = 0;
        for (uint32_t r = 0; r < m; r++) {
            if (asg[r]) continue;
            asg[r] = 1, fifo[tail++] = r, root[nb + r] = nb + r;
            while (head < tail) {
                const uint32_t p = fifo[head++];
                for (uint32_t c = 0; c < m; c++)
                    if (!asg[c] && grp_joins(s_umi[nb + p], s_cnt[nb + p], s_umi[nb + c], s_cnt[nb + c], edits))
                        asg[c] = 1, fifo[tail++] = c, root[nb + c] = nb + r;
            }
        }
    }
    // 5. ids, strands, the output order
    std::vector<int64_t> roff(nn + 1);
    int64_t nm = 0;
    for (size_t j = 0; j < nn; j++) roff[j] = nm, nm += root[j] == j;
    for (size_t i = 0; i < N; i++) {
        const uint32_t t = idx[i], r = root[npos[node_of[i]]];
        const uint32_t first = idx[nstart[nidx[r]]];
        mol[t] = (uint32_t)roff[r], ab[t] = (strand[t] & 1) != (strand[first] & 1);
        keys[t] = (uint64_t)roff[r] << 1 | ab[t];
        order[t] = t;
    }
    {
        int32_t mr, mp;
        grp_sort_bounds((uint64_t)nm << 1 | 1u, &mr, &mp);
        if (bsdc_zip_sort_host(keys.data(), order, n, mr, mp)) return grp_fail(std::string("bsdc_group_assign_host: ") + bsdc_zip_last_error());
    }
    stats[0] = (int64_t)ng, stats[1] = (int64_t)nn, stats[2] = nm, stats[3] = max_nodes;
    return 0;
}

int32_t bsdc_group_format_host(const uint32_t *order, const uint32_t *mol, const uint8_t *ab, int64_t n, const bsdc_group_rec *tab,
                               const uint8_t *rec, int64_t rec_bytes, const char *tag, int64_t *off, uint8_t *dst, int64_t cap) {
    GwArgs A;
    if (const int32_t rc = gw_check("bsdc_group_format_host", order, mol, ab, n, tab, tab, rec, rec, rec_bytes, tag, off, dst, cap, &A))
        return rc;
    for (int64_t k = 0; k < n; k++)
        if ((int64_t)order[k] >= n) return grp_fail("bsdc_group_format_host: order[" + std::to_string(k) + "] is not below n");
    int64_t o = 0;
    for (int64_t k = 0; k < 2 * n; k++) {
        const GwRec q = gw_rec(A, k);
        const int64_t size = gw_emit<false>(A, q, 0, 0, 0, 1);
        off[k] = o;
        gw_emit<true>(A, q, (uint32_t)size, o, 0, 1);
        o += size;
    }
    off[2 * n] = o;
    return 0;
}

#ifdef __HIPCC__
int64_t bsdc_group_tmp_bytes(int64_t n) {
    if (n < 0) return -1;
    return ga_carve(n, nullptr, nullptr, nullptr, nullptr) + 8;
}

int32_t bsdc_group_assign(const uint64_t *k0, const uint64_t *k1, const uint64_t *umi, const uint8_t *strand, int64_t n,
                          int32_t edits, const uint64_t *kmax, int32_t arena, uint32_t *mol, uint8_t *ab, uint32_t *order,
                          int64_t *stats, uint8_t *tmp, void *stream) {
    if (const int32_t rc = ga_check("bsdc_group_assign", k0, k1, umi, strand, n, edits, kmax, mol, ab, order, stats)) return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return grp_fail("bsdc_group_assign: tmp is null or not 8-byte aligned");
    if (arena < 0 || arena > 1) return grp_fail("bsdc_group_assign: arena is 0 (LDS while it fits) or 1 (scratch)");
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    GaArgs A;
    uint8_t *sort_tmp = nullptr;
    int64_t *bsum = nullptr;
    ga_carve(n, tmp, &A, &sort_tmp, &bsum);
    A.k0 = k0, A.k1 = k1, A.umi = umi, A.strand = strand, A.n = n, A.edits = edits;
    A.mol = mol, A.ab = ab, A.order = order, A.n_nodes = 0, A.n_groups = 0;
    auto fail = [&](const char *what) {
        (void)hipGetLastError();
        g_grp_err = std::string("bsdc_group_assign: ") + what;
        return BSDC_EDEVICE;
    };
    // bsdc_zip_sort's own code (BSDC_EINVAL or BSDC_EDEVICE) with its message
    auto sort = [&](uint64_t *keys, uint32_t *idx, int64_t cnt, uint64_t bound) {
        int32_t mr, mp;
        grp_sort_bounds(bound, &mr, &mp);
        const int32_t rc = bsdc_zip_sort(keys, idx, cnt, mr, mp, sort_tmp, stream);
        if (rc) g_grp_err = std::string("bsdc_group_assign: ") + bsdc_zip_last_error();
        return rc;
    };
    // 1.
    hipLaunchKernelGGL(k_grp_iota, dim3(blocks(n)), dim3(kT), 0, st, A.idx, n);
    const uint64_t *words[3] = {umi, k1, k0};
    for (int w = 0; w < 3; w++) {
        hipLaunchKernelGGL(k_grp_gather, dim3(blocks(n)), dim3(kT), 0, st, A.keys, words[w], A.idx, n);
        if (const int32_t rc = sort(A.keys, A.idx, n, kmax[2 - w])) return rc;
    }
    // 2.
    hipLaunchKernelGGL(k_grp_flags, dim3(blocks(n)), dim3(kT), 0, st, A);
    GsArgs S;
    S.f = A.flag, S.o = A.foff, S.n_fam = n, S.groups = scan_groups(n), S.bsum = bsum;
    launch_scan<2>(S, st);
    hipLaunchKernelGGL(k_grp_bounds, dim3(blocks(n)), dim3(kT), 0, st, A);
    int64_t tot[2] = {0, 0};
    if (hipMemcpyAsync(&tot[0], A.foff + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&tot[1], A.foff + 2 * n + 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("the group and node counts did not come back");
    A.n_groups = tot[0], A.n_nodes = tot[1];
    if (A.n_groups < 1 || A.n_groups > A.n_nodes || A.n_nodes > n) return fail("the group and node counts are out of range");
    // 3.
    hipLaunchKernelGGL(k_grp_nodekeys, dim3(blocks(A.n_nodes)), dim3(kT), 0, st, A);
    if (const int32_t rc = sort(A.nkeys, A.nidx, A.n_nodes, (uint64_t)(A.n_groups - 1) << 32 | (uint64_t)(uint32_t)n)) return rc;
    hipLaunchKernelGGL(k_grp_nodes, dim3(blocks(A.n_nodes)), dim3(kT), 0, st, A);
    // 4.
    uint32_t cnts[2] = {0, 0};
    if (hipMemsetAsync(A.counters, 0, 8, st) != hipSuccess) return fail("hipMemsetAsync failed");
    hipLaunchKernelGGL(k_group_small, dim3((unsigned)((A.n_groups + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, A);
    if (hipMemcpyAsync(cnts, A.counters, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("k_group_small failed");
    if ((int64_t)cnts[0] > A.n_groups) return fail("the list of large groups is out of range");
    if (cnts[0]) {
        const int lds_nodes = arena == 1 ? 0 : (int)std::min<int64_t>(kGrpLdsNodes, cnts[1]);
        hipLaunchKernelGGL(k_group_large, dim3(cnts[0]), dim3(kGrpLargeThreads), (size_t)lds_nodes * kGrpNodeBytes + 16, st, A,
                           lds_nodes);
    }
    // 5.
    hipLaunchKernelGGL(k_grp_isroot, dim3(blocks(A.n_nodes)), dim3(kT), 0, st, A);
    GsArgs R;
    R.f = A.isroot, R.o = A.roff, R.n_fam = A.n_nodes, R.groups = scan_groups(A.n_nodes), R.bsum = bsum;
    launch_scan<1>(R, st);
    int64_t nm = 0;
    if (hipMemcpyAsync(&nm, A.roff + A.n_nodes, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("the walk kernels failed");
    if (nm < A.n_groups || nm > A.n_nodes) return fail("the molecule count is out of range");
    hipLaunchKernelGGL(k_grp_number, dim3(blocks(n)), dim3(kT), 0, st, A);
    if (const int32_t rc = sort(A.keys, order, n, (uint64_t)nm << 1 | 1u)) return rc;
    if (hipGetLastError() != hipSuccess) return fail("a kernel launch failed");
    stats[0] = A.n_groups, stats[1] = A.n_nodes, stats[2] = nm, stats[3] = cnts[1] ? cnts[1] : 1;
    return 0;
}

int64_t bsdc_group_format_tmp_bytes(int64_t n) {
    if (n < 0) return -1;
    return (scan_groups(2 * n) + 1) * 8 + 2 * n * 4 + 8;
}

int32_t bsdc_group_format(const uint32_t *order, const uint32_t *mol, const uint8_t *ab, int64_t n, const bsdc_group_rec *tab,
                          const bsdc_group_rec *tab_host, const uint8_t *rec, const uint8_t *rec_host, int64_t rec_bytes,
                          const char *tag, int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream) {
    GwArgs A;
    if (const int32_t rc = gw_check("bsdc_group_format", order, mol, ab, n, tab, tab_host, rec, rec_host, rec_bytes, tag, off, dst,
                                    cap, &A))
        return rc;
    if (!tmp || ((uintptr_t)tmp & 7u)) return grp_fail("bsdc_group_format: tmp is null or not 8-byte aligned");
    A.groups = scan_groups(2 * n);
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    A.stat = reinterpret_cast<uint32_t *>(tmp + (A.groups + 1) * 8);
    hipStream_t st = (hipStream_t)stream;
    const unsigned wgs = (unsigned)((2 * n + kT / 64 - 1) / (kT / 64));
    if (wgs) hipLaunchKernelGGL(k_group_sizes, dim3(wgs), dim3(kT), 0, st, A);
    launch_scan<1>(A, st);
    if (wgs) hipLaunchKernelGGL(k_group_write, dim3(wgs), dim3(kT), 0, st, A);
    if (hipGetLastError() != hipSuccess) {
        g_grp_err = "bsdc_group_format: a kernel launch failed";
        return BSDC_EDEVICE;
    }
    return 0;
}
#endif

}  // extern "C"
