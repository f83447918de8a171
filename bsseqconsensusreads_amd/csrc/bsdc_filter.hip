// fgbio FilterConsensusReads on the GPU (gfx950), DESIGN.md sections 3.8 (the rules) and 5.5 (this
// kernel): a streaming pass over what a BSDC_MODE_TAGS run left in HBM -- the single-strand rows
// ss_* with their per-column depths and errors, and the consensus seq / qual, which it masks in
// place -- so filtered reads leave the device with no tag byte ever copied out.
//
// One wavefront per family (four per 256-thread workgroup), its two ends in turn: the template
// verdict (filt[f] = the OR of both ends' reasons) then needs no traffic between waves, and nothing
// here uses LDS or a barrier.  A lane owns 8 consecutive columns per round of 512: two dwords per
// ss_* byte row (four per u16 wide row), one dword of packed seq, two of qual, and whole-dword
// stores back (strides are multiples of 16, so every row is 16-byte aligned; columns at and past
// the read's length ride along unchanged).  Two sweeps per end: the per-read sums and maxima of the
// read-level gate (integer wave reductions by __shfl_xor), then, for an end that passed, the
// per-base mask with the no-call and mean-quality counts; the second sweep finds its rows in L2.
// The rows a / b of an end, the duplex column rule and the per-read rate are bsdc_ssrows.h's.
// Rates: the per-read ones are float32 divides (the tag encoder's, bsdc_ssrows.h read_rate; hipcc's
// default correctly rounded divide), the per-base ones fp64 divides, both compared in fp64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"
#include "bsdc_ssrows.h"

namespace bsdc_internal {  // csrc/bsdc_kernels.hip: the context's device and error text
int ctx_device(const bsdc_ctx *c);
int32_t ctx_fail(bsdc_ctx *c, int32_t code, const std::string &msg);
}  // namespace bsdc_internal

namespace {

constexpr int kCols = 8;             // columns a lane owns per round
constexpr int kRound = 64 * kCols;   // columns a wavefront covers per round
constexpr int kFilterWaves = 4;      // families per workgroup

struct FilterArgs {
    bsdc_filter_params p;
    int32_t kind, stride;
    int64_t n_fam;
    const uint8_t *status;
    const uint16_t *len;
    uint8_t *seq, *qual;
    const uint16_t *ss_len;
    const uint8_t *ss_base, *ss_qual, *ss_depth, *ss_err;
    const int32_t *ss_wide;
    const uint16_t *ss_wdepth, *ss_werr;
    uint8_t *filt;
    uint16_t *masked;
};

using bsdc_devtext::wave_max;
using bsdc_devtext::wave_sum;
using bsdc_ssrows::Row;  // one single-strand row (f, s)

// the lane's 8 columns from c0 (a multiple of 8) of a byte row / a u16 row
__device__ inline void load8(const uint8_t *p, int c0, uint32_t v[kCols]) {
    const uint2 w = *reinterpret_cast<const uint2 *>(p + c0);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = (w.x >> (8 * j)) & 255u;
        v[4 + j] = (w.y >> (8 * j)) & 255u;
    }
}
__device__ inline void load8w(const uint16_t *p, int c0, uint32_t v[kCols]) {
    const uint4 w = *reinterpret_cast<const uint4 *>(p + c0);
    v[0] = w.x & 0xFFFFu, v[1] = w.x >> 16, v[2] = w.y & 0xFFFFu, v[3] = w.y >> 16;
    v[4] = w.z & 0xFFFFu, v[5] = w.z >> 16, v[6] = w.w & 0xFFFFu, v[7] = w.w >> 16;
}
__device__ inline void load_counts(const Row &r, int c0, uint32_t d[kCols], uint32_t e[kCols]) {
    if (r.d16) {
        load8w(r.d16, c0, d);
        load8w(r.e16, c0, e);
    } else {
        load8(r.d8, c0, d);
        load8(r.e8, c0, e);
    }
}

__device__ inline double rate64(uint32_t e, uint32_t d) { return d ? (double)e / (double)d : 0.0; }
__device__ inline float nan0(float x) { return x != x ? 0.0f : x; }

// One end of one family: -> its reason bits; *n_masked = its newly masked columns.
__device__ int filter_end(const FilterArgs &A, int64_t f, int e, int lane, uint32_t *n_masked) {
    const bsdc_filter_params &p = A.p;
    const int L = min((int)A.len[2 * f + e], A.stride);
    const int32_t wide = A.ss_wide ? A.ss_wide[f] : -1;
    const bsdc_ssrows::End s = bsdc_ssrows::end_rows(A.kind, A.ss_len, f, e);
    const bool two = s.two;
    const Row a = bsdc_ssrows::row_of(A, f, s.a, wide), b = bsdc_ssrows::row_of(A, f, s.b, wide);

    // sweep 1: the per-read depths and error sums (all below 2^32: L <= 65535, counts <= 32767)
    uint32_t sad = 0, sae = 0, sbd = 0, sbe = 0, std_ = 0, ste = 0, mad = 0, mbd = 0, mcd = 0;
    for (int c0 = lane * kCols; c0 < L; c0 += kRound) {
        uint32_t ad[kCols], ae[kCols], bd[kCols], be[kCols], ab[kCols], aq[kCols], bb[kCols], bq[kCols];
        load_counts(a, c0, ad, ae);
        if (two) {
            load_counts(b, c0, bd, be);
            load8(a.b, c0, ab);
            load8(a.q, c0, aq);
            load8(b.b, c0, bb);
            load8(b.q, c0, bq);
        }
#pragma unroll
        for (int j = 0; j < kCols; j++) {
            if (c0 + j >= L) break;
            sad += ad[j];
            sae += ae[j];
            mad = max(mad, ad[j]);
            if (two) {
                sbd += bd[j];
                sbe += be[j];
                mbd = max(mbd, bd[j]);
                const bsdc_ssrows::Col c = bsdc_ssrows::duplex_col(ab[j], aq[j], ad[j], ae[j], bb[j], bq[j], bd[j], be[j]);
                std_ += c.d;
                ste += c.e;
                mcd = max(mcd, c.d);
            }
        }
    }
    sad = wave_sum(sad), sae = wave_sum(sae), mad = wave_max(mad);
    if (two) {
        sbd = wave_sum(sbd), sbe = wave_sum(sbe), mbd = wave_max(mbd);
        std_ = wave_sum(std_), ste = wave_sum(ste), mcd = wave_max(mcd);
    } else {
        std_ = sad, ste = sae, mcd = mad;
    }
    // the read-level gate (a NaN rate, no depth at all, never exceeds a threshold)
    using bsdc_ssrows::read_rate;
    const float aE = read_rate(sae, sad), cE = read_rate(ste, std_);
    const float bE = two ? read_rate(sbe, sbd) : 0.0f;
    int reason = 0;
    if ((int64_t)mcd < (int64_t)p.min_reads[0]) reason |= BSDC_FILT_MINREADS;
    if ((double)cE > p.max_read_error_rate[0]) reason |= BSDC_FILT_READERR;
    if (A.kind == 0) {
        if ((int64_t)max(mad, mbd) < (int64_t)p.min_reads[1] || (int64_t)min(mad, mbd) < (int64_t)p.min_reads[2])
            reason |= BSDC_FILT_MINREADS;
        const float x = nan0(aE), y = nan0(bE);
        if ((double)fminf(x, y) > p.max_read_error_rate[1] || (double)fmaxf(x, y) > p.max_read_error_rate[2])
            reason |= BSDC_FILT_READERR;
    }
    *n_masked = 0;
    if (reason) return reason;  // (not masked)

    // sweep 2: the per-base mask, in place, and the counts of the two checks after it
    uint8_t *const seq = A.seq + (size_t)(2 * f + e) * (size_t)(A.stride >> 1);
    uint8_t *const qual = A.qual + (size_t)(2 * f + e) * (size_t)A.stride;
    const bool agree = two && p.require_single_strand_agreement != 0;
    uint32_t n_n = 0, sq = 0, nm = 0;
    for (int c0 = lane * kCols; c0 < L; c0 += kRound) {
        uint32_t ad[kCols], ae[kCols], bd[kCols], be[kCols], ab[kCols], bb[kCols];
        load_counts(a, c0, ad, ae);
        if (two) load_counts(b, c0, bd, be);
        if (agree) {
            load8(a.b, c0, ab);
            load8(b.b, c0, bb);
        }
        uint32_t sw = *reinterpret_cast<const uint32_t *>(seq + (c0 >> 1));
        uint2 qw = *reinterpret_cast<const uint2 *>(qual + c0);
        bool changed = false;
#pragma unroll
        for (int j = 0; j < kCols; j++) {
            if (c0 + j >= L) break;
            const int ns = 8 * (j >> 1) + ((j & 1) ? 0 : 4);  // BAM packing: high nibble first
            const int qs = 8 * (j & 3);
            uint32_t base = (sw >> ns) & 15u;
            uint32_t q = ((j < 4 ? qw.x : qw.y) >> qs) & 255u;
            if (base != 15u) {
                bool m = (int)q < p.min_base_quality;
                if (A.kind == 1) {
                    m |= (int64_t)ad[j] < (int64_t)p.min_reads[0];
                    m |= rate64(ae[j], ad[j]) > p.max_base_error_rate[0];
                } else {
                    const uint32_t d2 = two ? bd[j] : 0u, e2 = two ? be[j] : 0u;
                    const uint32_t td = ad[j] + d2;
                    const double ra = rate64(ae[j], ad[j]), rb = rate64(e2, d2);
                    m |= (int64_t)td < (int64_t)p.min_reads[0];
                    m |= rate64(ae[j] + e2, td) > p.max_base_error_rate[0];
                    m |= (int64_t)max(ad[j], d2) < (int64_t)p.min_reads[1];
                    m |= (int64_t)min(ad[j], d2) < (int64_t)p.min_reads[2];
                    m |= fmin(ra, rb) > p.max_base_error_rate[1];
                    m |= fmax(ra, rb) > p.max_base_error_rate[2];
                    if (agree) m |= (ab[j] & 15u) != (bb[j] & 15u);
                }
                if (m) {
                    base = 15u, q = 2u;
                    sw |= 15u << ns;
                    if (j < 4)
                        qw.x = (qw.x & ~(255u << qs)) | (2u << qs);
                    else
                        qw.y = (qw.y & ~(255u << qs)) | (2u << qs);
                    nm++;
                    changed = true;
                }
            }
            n_n += base == 15u;
            sq += q;
        }
        if (changed) {
            *reinterpret_cast<uint32_t *>(seq + (c0 >> 1)) = sw;
            *reinterpret_cast<uint2 *>(qual + c0) = qw;
        }
    }
    n_n = wave_sum(n_n), sq = wave_sum(sq), nm = wave_sum(nm);
    *n_masked = nm;
    if ((double)n_n / (double)L > p.max_no_call_fraction) reason |= BSDC_FILT_NOCALL;  // (L = 0: NaN, kept)
    if (p.min_mean_base_quality >= 0 && (int64_t)sq < (int64_t)p.min_mean_base_quality * (int64_t)L)
        reason |= BSDC_FILT_MEANQ;
    return reason;
}

__global__ __launch_bounds__(64 * kFilterWaves) void k_filter(const FilterArgs A) {
    const int64_t f = (int64_t)blockIdx.x * kFilterWaves + (threadIdx.x >> 6);
    if (f >= A.n_fam) return;
    const int lane = threadIdx.x & 63;
    int reason = 0;
    uint32_t nm[2] = {0, 0};
    if (A.status[f] & 1) {  // (a family that is not emitted is not looked at)
        reason = filter_end(A, f, 0, lane, &nm[0]);
        reason |= filter_end(A, f, 1, lane, &nm[1]);
    }
    if (lane == 0) {
        A.filt[f] = (uint8_t)reason;
        A.masked[2 * f] = (uint16_t)nm[0];
        A.masked[2 * f + 1] = (uint16_t)nm[1];
    }
}

// nullptr inside the supported domain (include/bsdc.h bsdc_filter_params), else the refusal
const char *filter_params_error(const bsdc_filter_params *p) {
    for (int k = 0; k < 3; k++) {
        if (p->min_reads[k] < 0) return "bad filter params: min_reads is negative";
        if (k && p->min_reads[k] > p->min_reads[k - 1])
            return "bad filter params: min_reads must not increase (duplex >= AB >= BA)";
        // (NaN fails both comparisons)
        if (!(p->max_read_error_rate[k] >= 0.0 && p->max_read_error_rate[k] <= 1.0))
            return "bad filter params: max_read_error_rate outside [0, 1]";
        if (!(p->max_base_error_rate[k] >= 0.0 && p->max_base_error_rate[k] <= 1.0))
            return "bad filter params: max_base_error_rate outside [0, 1]";
    }
    if (p->min_base_quality < 0 || p->min_base_quality > 93) return "bad filter params: min_base_quality outside 0..93";
    if (!(p->max_no_call_fraction >= 0.0 && p->max_no_call_fraction <= 1.0))
        return "bad filter params: max_no_call_fraction outside [0, 1]";
    if (p->min_mean_base_quality < -1 || p->min_mean_base_quality > 93)
        return "bad filter params: min_mean_base_quality outside -1..93";
    return nullptr;
}

}  // namespace

extern "C" int32_t bsdc_filter(bsdc_ctx *c, const bsdc_filter_params *params, int32_t kind, int64_t n_fam,
                               bsdc_consensus *o, uint8_t *filt, uint16_t *masked, void *stream) {
    using bsdc_internal::ctx_fail;
    if (!c) return BSDC_EINVAL;
    if (!params || !o || !filt || !masked || n_fam < 0 || (kind != 0 && kind != 1))
        return ctx_fail(c, BSDC_EINVAL, "bsdc_filter: null argument, negative n_fam or kind outside 0..1");
    if (const char *why = filter_params_error(params)) return ctx_fail(c, BSDC_EINVAL, why);
    if (!o->status || !o->len || !o->seq || !o->qual) return ctx_fail(c, BSDC_EINVAL, "bsdc_filter: output buffers missing");
    if (!o->ss_len || !o->ss_base || !o->ss_qual || !o->ss_depth || !o->ss_err)
        return ctx_fail(c, BSDC_EINVAL, "bsdc_filter needs the ss_* rows of a BSDC_MODE_TAGS run");
    if (o->ss_wide && (!o->ss_wdepth || !o->ss_werr)) return ctx_fail(c, BSDC_EINVAL, "ss_wide needs ss_wdepth and ss_werr");
    // the lanes' dword loads and stores: rows a multiple of 16 long, from 16-byte aligned bases
    if (o->stride < 16 || (o->stride & 15)) return ctx_fail(c, BSDC_EINVAL, "stride must be a positive multiple of 16");
    const uintptr_t bases = (uintptr_t)o->seq | (uintptr_t)o->qual | (uintptr_t)o->ss_base | (uintptr_t)o->ss_qual |
                            (uintptr_t)o->ss_depth | (uintptr_t)o->ss_err | (uintptr_t)o->ss_wdepth | (uintptr_t)o->ss_werr;
    if (bases & 15) return ctx_fail(c, BSDC_EINVAL, "bsdc_filter: seq, qual and the ss_* rows must be 16-byte aligned");
    const int64_t blocks = (n_fam + kFilterWaves - 1) / kFilterWaves;
    if (blocks > 0x7FFFFFFF) return ctx_fail(c, BSDC_EINVAL, "bsdc_filter: too many families for one launch");
    if (n_fam == 0) return 0;
    hipError_t e = hipSetDevice(bsdc_internal::ctx_device(c));
    if (e != hipSuccess) return ctx_fail(c, BSDC_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    FilterArgs A;
    A.p = *params;
    A.kind = kind, A.stride = o->stride, A.n_fam = n_fam;
    A.status = o->status, A.len = o->len, A.seq = o->seq, A.qual = o->qual;
    A.ss_len = o->ss_len, A.ss_base = o->ss_base, A.ss_qual = o->ss_qual, A.ss_depth = o->ss_depth, A.ss_err = o->ss_err;
    A.ss_wide = o->ss_wide, A.ss_wdepth = o->ss_wdepth, A.ss_werr = o->ss_werr;
    A.filt = filt, A.masked = masked;
    hipLaunchKernelGGL(k_filter, dim3((unsigned)blocks), dim3(64 * kFilterWaves), 0, reinterpret_cast<hipStream_t>(stream), A);
    e = hipGetLastError();
    if (e != hipSuccess) return ctx_fail(c, BSDC_EDEVICE, std::string("k_filter launch: ") + hipGetErrorString(e));
    return 0;
}
