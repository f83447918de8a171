// Per-run consensus metrics on the GPU (gfx950), DESIGN.md sections 3.9 (the definitions) and 8.10
// (this kernel): one reduction over what a BSDC_MODE_TAGS run left in HBM -- the single-strand rows
// with their per-column depths and errors and the unfiltered consensus seq / qual -- into an
// accumulator of u64 counters (include/bsdc.h bsdc_metrics_words): the distributions of fgbio's
// consensus tags that a user picks the filter's thresholds from, with no tag byte copied out.
//
// A fixed number of 256-thread workgroups strides over the families, one wavefront per family, its
// two ends in turn (the views a / b and the per-read rate are bsdc_ssrows.h's; its
// duplex column rule is written out in met_record, for the kernel's speed).  A lane
// owns 4 consecutive columns per round of 256: one dword per byte row, two per u16 wide row, one
// 16-bit word of packed seq, one dword of qual (strides are multiples of 16, rows 16-byte aligned).
// All tables live in LDS as u32, added to with LDS atomics: the three histograms, and by_cycle
// counter-major ([end][counter][column], the column index swizzled so that the 64 lanes of one add
// hit 64 banks).  Columns at and past cycles - 1 share the accumulator's last row: they add into
// twelve u64 LDS words.  Per-read sums and maxima are integer wave reductions by __shfl_xor.  Each
// workgroup flushes once at its end (and after every 32768 families, which keeps the u32 tables
// from wrapping) with one 64-bit global atomic add per non-zero word; integer adds commute, so the
// result does not depend on the order.  No per-column global atomics.
// Bounds: a family whose length exceeds the stride or whose wide row lies outside [0, n_wide) is
// counted as skipped and none of its rows is read.
// The per-record function is __host__ __device__: bsdc_metrics_host runs it sequentially on the CPU
// with one "lane" and plain adds; built without hipcc this file holds that twin alone
// (tests/sanitize/metrics_twin_main.cpp).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"
#include "bsdc_ssrows.h"

#ifdef __HIPCC__
#define MET_UNROLL _Pragma("unroll")
namespace bsdc_internal {  // csrc/bsdc_kernels.hip: the context's device and error text
int ctx_device(const bsdc_ctx *c);
int32_t ctx_fail(bsdc_ctx *c, int32_t code, const std::string &msg);
}  // namespace bsdc_internal
#else
#define MET_UNROLL
#endif

namespace {

constexpr int kMetCols = 4;                   // columns a lane owns per round
constexpr int kMetWaves = 4;                  // families a workgroup works on at a time
constexpr int kMetT = 64 * kMetWaves;
constexpr int kMetGrid = 768;                 // workgroups of a launch (256 CUs x 3 resident)
constexpr int kMetFlushEvery = 8192;          // rounds of kMetWaves families between two flushes
constexpr int kMetMaxCycles = 1024;           // 12 * cycles u32 of LDS, below 64 KiB

// the accumulator's layout (include/bsdc.h)
constexpr int kOffDepth = BSDC_METRICS_DEPTH_HIST, kOffRate = BSDC_METRICS_RATE_HIST;
constexpr int kOffQual = BSDC_METRICS_QUAL_HIST, kOffCycle = BSDC_METRICS_BY_CYCLE;
constexpr int kHistWords = kOffCycle - kOffDepth;  // the three histograms, contiguous

struct MetArgs {
    int32_t kind, stride, cycles;
    int64_t n_fam, n_wide;
    const uint8_t *status;
    const uint16_t *len;
    const uint8_t *seq, *qual;
    const uint16_t *ss_len;
    const uint8_t *ss_base, *ss_qual, *ss_depth, *ss_err;
    const int32_t *ss_wide;
    const uint16_t *ss_wdepth, *ss_werr;
};

using bsdc_ssrows::Row;  // one single-strand row (f, s)

// aligned little-endian loads (the twin copies: no alignment assumed of a host caller's casts)
BSDC_HD uint32_t met_ld32(const void *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
BSDC_HD uint32_t met_ld16(const void *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint16_t *>(p);
#else
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
#endif
}

// the lane's 4 columns from c0 (a multiple of 4) of a byte row / of the depths and errors
BSDC_HD void met_ld4(const uint8_t *p, int c0, uint32_t v[kMetCols]) {
    const uint32_t w = met_ld32(p + c0);
    v[0] = w & 255u, v[1] = (w >> 8) & 255u, v[2] = (w >> 16) & 255u, v[3] = w >> 24;
}
BSDC_HD void met_counts(const Row &r, int c0, uint32_t d[kMetCols], uint32_t e[kMetCols]) {
    if (r.d16) {
        const uint32_t d0 = met_ld32(r.d16 + c0), d1 = met_ld32(r.d16 + c0 + 2);
        const uint32_t e0 = met_ld32(r.e16 + c0), e1 = met_ld32(r.e16 + c0 + 2);
        d[0] = d0 & 0xFFFFu, d[1] = d0 >> 16, d[2] = d1 & 0xFFFFu, d[3] = d1 >> 16;
        e[0] = e0 & 0xFFFFu, e[1] = e0 >> 16, e[2] = e1 & 0xFFFFu, e[3] = e1 >> 16;
    } else {
        met_ld4(r.d8, c0, d);
        met_ld4(r.e8, c0, e);
    }
}

// bin of a per-read error rate: floor(x * 1000) capped at 100 (an infinite rate too), NaN -> 101
BSDC_HD int met_rate_bin(float x) {
    if (x != x) return 101;
    const double t = (double)x * 1000.0;
    return t >= 100.0 ? 100 : (int)floor(t);
}

BSDC_HD bool met_acgt(uint32_t x) { return x == 1u || x == 2u || x == 4u || x == 8u; }

// 0, or why family f is skipped: 1 a length beyond the stride, 2 a wide row outside the table
BSDC_HD int met_family_check(const MetArgs &A, int64_t f, int32_t *wide) {
    *wide = A.ss_wide ? A.ss_wide[f] : -1;
    if ((int)A.len[2 * f] > A.stride || (int)A.len[2 * f + 1] > A.stride) return 1;
    if (*wide >= 0 && (int64_t)*wide >= A.n_wide) return 2;
    return 0;
}

// One output record (family f, end e) into the sink S: hist(word) adds 1 to a histogram word
// (offset from the accumulator's depth_hist), cyc(e, c, k, v) adds v to by_cycle[e][min(c, cycles -
// 1)][k], sum / max reduce over the sink's lanes.  `lane` of S::kLanes takes columns 4 lane .. 4
// lane + 3 of every round.
template <class S>
BSDC_HD void met_record(const MetArgs &A, int64_t f, int e, int32_t wide, int lane, S &sink) {
    const int L = (int)A.len[2 * f + e];
    const bsdc_ssrows::End s = bsdc_ssrows::end_rows(A.kind, A.ss_len, f, e);
    const bool two = s.two;
    const Row a = bsdc_ssrows::row_of(A, f, s.a, wide), b = bsdc_ssrows::row_of(A, f, s.b, wide);
    const uint8_t *const seq = A.seq + (size_t)(2 * f + e) * (size_t)(A.stride >> 1);
    const uint8_t *const qual = A.qual + (size_t)(2 * f + e) * (size_t)A.stride;

    // (sums below 2^32: L <= 65535, counts <= 32767 a strand)
    uint32_t sad = 0, sae = 0, sbd = 0, sbe = 0, std_ = 0, ste = 0, mad = 0, mbd = 0, mcd = 0;
    for (int c0 = lane * kMetCols; c0 < L; c0 += S::kLanes * kMetCols) {
        uint32_t ad[kMetCols], ae[kMetCols], bd[kMetCols] = {0, 0, 0, 0}, be[kMetCols] = {0, 0, 0, 0};
        uint32_t ab[kMetCols] = {0, 0, 0, 0}, aq[kMetCols] = {0, 0, 0, 0}, bb[kMetCols] = {0, 0, 0, 0},
                 bq[kMetCols] = {0, 0, 0, 0};
        met_counts(a, c0, ad, ae);
        if (two) {
            met_counts(b, c0, bd, be);
            met_ld4(a.b, c0, ab);
            met_ld4(a.q, c0, aq);
            met_ld4(b.b, c0, bb);
            met_ld4(b.q, c0, bq);
        }
        const uint32_t sw = met_ld16(seq + (c0 >> 1));
        const uint32_t qw = met_ld32(qual + c0);
        MET_UNROLL
        for (int j = 0; j < kMetCols; j++) {
            const int c = c0 + j;
            if (c >= L) break;
            sad += ad[j];
            sae += ae[j];
            mad = mad > ad[j] ? mad : ad[j];
            uint32_t dis = 0;
            if (two) {
                sbd += bd[j];
                sbe += be[j];
                mbd = mbd > bd[j] ? mbd : bd[j];
                // bsdc_ssrows::duplex_col, written out: through the call k_metrics came out with 28
                // more exec-mask branches and ran 4.5% slower (0.785 against 0.751 ms, 200k families)
                const uint32_t x = ab[j] & 15u, y = bb[j] & 15u;
                const uint32_t raw = x == y ? x : aq[j] > bq[j] ? x : bq[j] > aq[j] ? y : x;
                const uint32_t td = ad[j] + bd[j];
                std_ += td;
                ste += (x == raw ? ae[j] : ad[j]) + (y == raw ? be[j] : bd[j]);
                mcd = mcd > td ? mcd : td;
                dis = met_acgt(x) && met_acgt(y) && x != y;
            }
            // the consensus column: BAM packing, high nibble first
            const uint32_t byte = (sw >> (8 * (j >> 1))) & 255u;
            const uint32_t base = (j & 1) ? (byte & 15u) : (byte >> 4);
            const uint32_t q = (qw >> (8 * j)) & 255u;
            const bool n = base == 15u;
            sink.hist((kOffQual - kOffDepth) + e * 95 + (n ? 94 : (int)(q < 93u ? q : 93u)));
            sink.cyc(e, c, 0, 1u);
            if (n) sink.cyc(e, c, 1, 1u);
            sink.cyc(e, c, 2, q);
            sink.cyc(e, c, 3, ad[j] + bd[j]);
            sink.cyc(e, c, 4, ae[j] + be[j]);
            if (dis) sink.cyc(e, c, 5, 1u);
        }
    }
    sad = sink.sum(sad), sae = sink.sum(sae), mad = sink.max(mad);
    if (two) {
        sbd = sink.sum(sbd), sbe = sink.sum(sbe), mbd = sink.max(mbd);
        std_ = sink.sum(std_), ste = sink.sum(ste), mcd = sink.max(mcd);
    } else {
        std_ = sad, ste = sae, mcd = mad;
    }
    if (lane != 0) return;
    // the per-read values as the tag encoder writes them: float32 divides, NaN with no depth
    using bsdc_ssrows::read_rate;
    const float aE = read_rate(sae, sad), cE = read_rate(ste, std_);
    const float bE = two ? read_rate(sbe, sbd) : 0.0f;
    const uint32_t D[3] = {mcd, mad, two ? mbd : 0u};
    const float E[3] = {cE, aE, bE};
    for (int k = 0; k < 3; k++) {
        sink.hist((k * 2 + e) * 256 + (int)(D[k] < 255u ? D[k] : 255u));
        sink.hist((kOffRate - kOffDepth) + (k * 2 + e) * 102 + met_rate_bin(E[k]));
    }
}

// the twin's sink: one lane, plain adds into the accumulator
struct HostSink {
    static constexpr int kLanes = 1;
    uint64_t *acc;
    int32_t cycles;
    inline uint32_t sum(uint32_t v) const { return v; }
    inline uint32_t max(uint32_t v) const { return v; }
    inline void hist(int w) { acc[kOffDepth + w] += 1; }
    inline void cyc(int e, int c, int k, uint32_t v) {
        const int r = c < cycles - 1 ? c : cycles - 1;
        acc[kOffCycle + ((size_t)e * cycles + r) * 6 + k] += v;
    }
};

thread_local std::string g_met_err;

int32_t met_fail(bsdc_ctx *c, const std::string &m) {
    g_met_err = m;
#ifdef __HIPCC__
    if (c) bsdc_internal::ctx_fail(c, BSDC_EINVAL, m);
#else
    (void)c;
#endif
    return BSDC_EINVAL;
}

// the arguments, as the launcher and the twin both refuse them; fills A
int32_t met_check(bsdc_ctx *c, const char *who, const bsdc_consensus *o, int64_t n_fam, int64_t n_wide, int32_t molecular,
                  int32_t cycles, const uint64_t *acc, MetArgs *A) {
    const std::string w(who);
    if (!o) return met_fail(c, w + ": out is null");
    if (!acc) return met_fail(c, w + ": acc is null");
    if (((uintptr_t)acc & 7u)) return met_fail(c, w + ": acc must be 8-byte aligned");
    if (n_fam < 0) return met_fail(c, w + ": n_fam is negative");
    if (n_wide < 0) return met_fail(c, w + ": n_wide is negative");
    if (molecular != 0 && molecular != 1) return met_fail(c, w + ": molecular outside 0..1");
    if (cycles < 2 || cycles > kMetMaxCycles) return met_fail(c, w + ": cycles outside 2.." + std::to_string(kMetMaxCycles));
    if (o->stride < 16 || (o->stride & 15)) return met_fail(c, w + ": stride must be a positive multiple of 16");
    if (!o->status) return met_fail(c, w + ": status is null");
    if (!o->len) return met_fail(c, w + ": len is null");
    if (!o->seq) return met_fail(c, w + ": seq is null");
    if (!o->qual) return met_fail(c, w + ": qual is null");
    if (!o->ss_len) return met_fail(c, w + ": ss_len is null (the rows of a BSDC_MODE_TAGS run)");
    if (!o->ss_base) return met_fail(c, w + ": ss_base is null (the rows of a BSDC_MODE_TAGS run)");
    if (!o->ss_qual) return met_fail(c, w + ": ss_qual is null (the rows of a BSDC_MODE_TAGS run)");
    if (!o->ss_depth) return met_fail(c, w + ": ss_depth is null (the rows of a BSDC_MODE_TAGS run)");
    if (!o->ss_err) return met_fail(c, w + ": ss_err is null (the rows of a BSDC_MODE_TAGS run)");
    if (o->ss_wide && n_wide > 0 && (!o->ss_wdepth || !o->ss_werr))
        return met_fail(c, w + ": ss_wide needs ss_wdepth and ss_werr");
    // the lanes' loads: a dword of every byte row and of the wide rows, a 16-bit word of seq
    const uintptr_t bases = (uintptr_t)o->qual | (uintptr_t)o->ss_base | (uintptr_t)o->ss_qual | (uintptr_t)o->ss_depth |
                            (uintptr_t)o->ss_err | (uintptr_t)o->ss_wdepth | (uintptr_t)o->ss_werr | (uintptr_t)o->seq |
                            (uintptr_t)o->len | (uintptr_t)o->ss_len | (uintptr_t)o->ss_wide;
    if (bases & 3) return met_fail(c, w + ": the consensus and ss_* buffers must be 4-byte aligned");
    A->kind = molecular, A->stride = o->stride, A->cycles = cycles, A->n_fam = n_fam, A->n_wide = n_wide;
    A->status = o->status, A->len = o->len, A->seq = o->seq, A->qual = o->qual;
    A->ss_len = o->ss_len, A->ss_base = o->ss_base, A->ss_qual = o->ss_qual, A->ss_depth = o->ss_depth, A->ss_err = o->ss_err;
    A->ss_wide = o->ss_wide, A->ss_wdepth = o->ss_wdepth, A->ss_werr = o->ss_werr;
    return 0;
}

int32_t met_filter_check(bsdc_ctx *c, const char *who, const uint8_t *status, const uint8_t *filt, const uint16_t *masked,
                         int64_t n_fam, const uint64_t *acc) {
    const std::string w(who);
    if (!status) return met_fail(c, w + ": status is null");
    if (!filt) return met_fail(c, w + ": filt is null");
    if (!masked) return met_fail(c, w + ": masked is null");
    if (!acc || ((uintptr_t)acc & 7u)) return met_fail(c, w + ": acc is null or not 8-byte aligned");
    if (n_fam < 0) return met_fail(c, w + ": n_fam is negative");
    return 0;
}

#ifdef __HIPCC__
// by_cycle column r's place in its LDS row: the four lanes 16 apart that one add would send to one
// bank (columns 64 apart) get four different ones
__device__ __forceinline__ int met_swz(int r) { return r ^ ((r >> 6) & 3); }

struct DevSink {
    static constexpr int kLanes = 64;
    uint32_t *hist32, *cyc32;
    unsigned long long *ovf;
    int32_t cycles, cyc4;
    __device__ __forceinline__ uint32_t sum(uint32_t v) const { return bsdc_devtext::wave_sum(v); }
    __device__ __forceinline__ uint32_t max(uint32_t v) const { return bsdc_devtext::wave_max(v); }
    __device__ __forceinline__ void hist(int w) { atomicAdd(&hist32[w], 1u); }
    __device__ __forceinline__ void cyc(int e, int c, int k, uint32_t v) {
        if (c < cycles - 1)
            atomicAdd(&cyc32[(e * 6 + k) * cyc4 + met_swz(c)], v);
        else
            atomicAdd(&ovf[e * 6 + k], (unsigned long long)v);
    }
};

// LDS: ovf u64 [12] | hist u32 [kHistWords] | cnt u32 [4] | cyc u32 [12][cyc4]
__host__ __device__ inline int met_cyc4(int cycles) { return (cycles + 3) & ~3; }
inline size_t met_lds_bytes(int cycles) { return 12 * 8 + 4 * ((size_t)kHistWords + 4 + 12 * (size_t)met_cyc4(cycles)); }

// the workgroup's tables into the accumulator (one 64-bit atomic add per non-zero word), then zeroed
__device__ void met_flush(const MetArgs &A, unsigned long long *acc, unsigned long long *ovf, uint32_t *hist32,
                          uint32_t *cnt, uint32_t *cyc32, int cyc4) {
    __syncthreads();
    const int t = threadIdx.x;
    for (int i = t; i < kHistWords; i += kMetT) {
        const uint32_t v = hist32[i];
        if (v) atomicAdd(&acc[kOffDepth + i], (unsigned long long)v);
        hist32[i] = 0;
    }
    if (t < 4) {
        if (cnt[t]) atomicAdd(&acc[t], (unsigned long long)cnt[t]);
        cnt[t] = 0;
    }
    const int C = A.cycles;
    for (int i = t; i < 12 * C; i += kMetT) {
        const int e = i / (6 * C), r = (i / 6) % C, k = i % 6;
        const unsigned long long v = r < C - 1 ? (unsigned long long)cyc32[(e * 6 + k) * cyc4 + met_swz(r)] : ovf[e * 6 + k];
        if (v) atomicAdd(&acc[kOffCycle + i], v);
    }
    __syncthreads();
    for (int i = t; i < 12 * cyc4; i += kMetT) cyc32[i] = 0;
    if (t < 12) ovf[t] = 0;
    __syncthreads();
}

__global__ __launch_bounds__(kMetT) void k_metrics(const MetArgs A, unsigned long long *acc) {
    extern __shared__ unsigned long long met_lds[];
    unsigned long long *const ovf = met_lds;
    uint32_t *const hist32 = reinterpret_cast<uint32_t *>(met_lds + 12);
    uint32_t *const cnt = hist32 + kHistWords;
    uint32_t *const cyc32 = cnt + 4;
    const int cyc4 = met_cyc4(A.cycles);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < kHistWords + 4 + 12 * cyc4; i += kMetT) hist32[i] = 0;
    if (t < 12) ovf[t] = 0;
    __syncthreads();
    DevSink sink{hist32, cyc32, ovf, A.cycles, cyc4};
    int rounds = 0;
    // (the trip count depends on the workgroup alone: the barriers of a flush are met by every wave)
    for (int64_t base = (int64_t)blockIdx.x * kMetWaves; base < A.n_fam; base += (int64_t)gridDim.x * kMetWaves) {
        const int64_t f = base + wave;
        if (f < A.n_fam) {
            const bool emitted = A.status[f] & 1;
            int32_t wide = -1;
            const int bad = emitted ? met_family_check(A, f, &wide) : 0;
            if (lane == 0) {
                atomicAdd(&cnt[BSDC_METRICS_FAMILIES], 1u);
                if (emitted) atomicAdd(&cnt[BSDC_METRICS_EMITTED], 1u);
                if (emitted && bad) atomicAdd(&cnt[BSDC_METRICS_SKIPPED], 1u);
                if (emitted && !bad) atomicAdd(&cnt[BSDC_METRICS_RECORDS], 2u);
            }
            if (emitted && !bad) {
#pragma nounroll
                for (int e = 0; e < 2; e++) met_record(A, f, e, wide, lane, sink);
            }
        }
        if (++rounds == kMetFlushEvery) {
            met_flush(A, acc, ovf, hist32, cnt, cyc32, cyc4);
            rounds = 0;
        }
    }
    met_flush(A, acc, ovf, hist32, cnt, cyc32, cyc4);
}

// the filter's outcome: families kept, one counter per reason bit, the masked columns
__global__ __launch_bounds__(256) void k_metrics_filter(const uint8_t *status, const uint8_t *filt, const uint16_t *masked,
                                                        int64_t n_fam, unsigned long long *acc) {
    uint32_t v[5] = {0, 0, 0, 0, 0};  // kept and the four reasons
    uint64_t nm = 0;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < n_fam; f += (int64_t)gridDim.x * 256) {
        if (!(status[f] & 1)) continue;
        const uint32_t r = filt[f];
        v[0] += r == 0;
        for (int k = 0; k < 4; k++) v[1 + k] += (r >> k) & 1u;
        nm += (uint64_t)masked[2 * f] + masked[2 * f + 1];
    }
    for (int k = 0; k < 5; k++) v[k] = bsdc_devtext::wave_sum(v[k]);
    nm = bsdc_devtext::wave_sum(nm);
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 5; k++)
            if (v[k]) atomicAdd(&acc[BSDC_METRICS_KEPT + k], (unsigned long long)v[k]);
        if (nm) atomicAdd(&acc[BSDC_METRICS_MASKED], (unsigned long long)nm);
    }
}
#endif

}  // namespace

extern "C" {

const char *bsdc_metrics_last_error(void) { return g_met_err.c_str(); }

int64_t bsdc_metrics_words(int32_t cycles) {
    if (cycles < 2 || cycles > kMetMaxCycles) return BSDC_EINVAL;
    return (int64_t)kOffCycle + 12 * (int64_t)cycles;
}

int32_t bsdc_metrics_host(bsdc_ctx *ctx, const bsdc_consensus *out, int64_t n_fam, int64_t n_wide, int32_t molecular,
                          int32_t cycles, uint64_t *acc) {
    MetArgs A;
    if (const int32_t rc = met_check(ctx, "bsdc_metrics_host", out, n_fam, n_wide, molecular, cycles, acc, &A)) return rc;
    HostSink sink{acc, cycles};
    for (int64_t f = 0; f < n_fam; f++) {
        acc[BSDC_METRICS_FAMILIES] += 1;
        if (!(A.status[f] & 1)) continue;
        acc[BSDC_METRICS_EMITTED] += 1;
        int32_t wide = -1;
        if (met_family_check(A, f, &wide)) {
            acc[BSDC_METRICS_SKIPPED] += 1;
            continue;
        }
        acc[BSDC_METRICS_RECORDS] += 2;
        met_record(A, f, 0, wide, 0, sink);
        met_record(A, f, 1, wide, 0, sink);
    }
    return 0;
}

int32_t bsdc_metrics_filter_host(bsdc_ctx *ctx, const uint8_t *status, const uint8_t *filt, const uint16_t *masked,
                                 int64_t n_fam, uint64_t *acc) {
    if (const int32_t rc = met_filter_check(ctx, "bsdc_metrics_filter_host", status, filt, masked, n_fam, acc)) return rc;
    for (int64_t f = 0; f < n_fam; f++) {
        if (!(status[f] & 1)) continue;
        acc[BSDC_METRICS_KEPT] += filt[f] == 0;
        for (int k = 0; k < 4; k++) acc[BSDC_METRICS_MINREADS + k] += (filt[f] >> k) & 1u;
        acc[BSDC_METRICS_MASKED] += (uint64_t)masked[2 * f] + masked[2 * f + 1];
    }
    return 0;
}

#ifdef __HIPCC__
int32_t bsdc_metrics(bsdc_ctx *ctx, const bsdc_consensus *out, int64_t n_fam, int64_t n_wide, int32_t molecular,
                     int32_t cycles, uint64_t *acc, void *stream) {
    if (!ctx) return met_fail(nullptr, "bsdc_metrics: null context");
    MetArgs A;
    if (const int32_t rc = met_check(ctx, "bsdc_metrics", out, n_fam, n_wide, molecular, cycles, acc, &A)) return rc;
    if (n_fam == 0) return 0;
    hipError_t e = hipSetDevice(bsdc_internal::ctx_device(ctx));
    if (e != hipSuccess) return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    const int64_t want = (n_fam + kMetWaves - 1) / kMetWaves;
    const unsigned grid = (unsigned)(want < kMetGrid ? want : kMetGrid);
    hipLaunchKernelGGL(k_metrics, dim3(grid), dim3(kMetT), met_lds_bytes(cycles), reinterpret_cast<hipStream_t>(stream), A,
                       reinterpret_cast<unsigned long long *>(acc));
    e = hipGetLastError();
    if (e != hipSuccess) return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("k_metrics launch: ") + hipGetErrorString(e));
    return 0;
}

int32_t bsdc_metrics_filter(bsdc_ctx *ctx, const uint8_t *status, const uint8_t *filt, const uint16_t *masked, int64_t n_fam,
                            uint64_t *acc, void *stream) {
    if (!ctx) return met_fail(nullptr, "bsdc_metrics_filter: null context");
    if (const int32_t rc = met_filter_check(ctx, "bsdc_metrics_filter", status, filt, masked, n_fam, acc)) return rc;
    if (n_fam == 0) return 0;
    hipError_t e = hipSetDevice(bsdc_internal::ctx_device(ctx));
    if (e != hipSuccess) return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    const int64_t want = (n_fam + 255) / 256;
    const unsigned grid = (unsigned)(want < 256 ? want : 256);
    hipLaunchKernelGGL(k_metrics_filter, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), status, filt, masked,
                       n_fam, reinterpret_cast<unsigned long long *>(acc));
    e = hipGetLastError();
    if (e != hipSuccess)
        return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("k_metrics_filter launch: ") + hipGetErrorString(e));
    return 0;
}
#endif

}  // extern "C"
