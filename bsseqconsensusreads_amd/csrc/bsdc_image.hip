// The family images gathered on the GPU (gfx950) from the records' SEQ and QUAL bytes as they lie in
// the BAM (include/bsdc.h bsdc_image_gather): what bsdc_materialize_fill and
// bsdc_split_move (csrc/bsdc_host.cpp) build on the host from unpacked bases.
//
// BAM's SEQ is already the image's nibble code, high nibble first; a record's kept bases
// skip .. skip + len - 1 go to nibbles slot + 1 .. slot + len of the packed image and its quals to
// the same bytes of the qual image, everything else is zero.  The launcher zeroes both images on
// the stream (two memsets) and k_image_gather then writes base bytes only:
//  * 16 lanes per record (four records a wavefront, 16 a workgroup): a record of 150 bases has 38
//    qual dwords and 19 or 20 seq dwords, four rounds of its 16 lanes; no scan over the table.
//  * a lane owns one ALIGNED dword of a destination at a time, builds it in a register and stores
//    it whole.  Qual: the four source bytes start at any byte of `raw`: two aligned dwords, funnel
//    shift by 8 * (address & 3).  Seq: the eight source nibbles start at any nibble (the byte
//    offset of SEQ, and the parity of skip, against nibble 1 of the slot): the two aligned source
//    dwords are byte-swapped, so that the first base is the top nibble, shifted by 4 * (nibble
//    address & 7), masked to the record's bases and swapped back.
//  * slots are 4 entries long-aligned: a qual dword always lies inside one record's slot; a dword
//    of the packed image (8 nibbles) can hold the end of one slot and the start of the next, and
//    then leaves as the one 16-bit half that is the record's own.  Two records never share a byte.
// Bounds: the kernel checks every table entry itself (img_rec_check, the launcher's test) and
// skips a bad one; sources are read by dwords that lie inside [0, n_raw) (the last partial one byte
// by byte), destinations written inside the images.  The host twin bsdc_image_gather_host runs the
// same per-dword function sequentially; built without hipcc this file holds the twin alone
// (tests/sanitize/image_twin_main.cpp).
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"  // BSDC_HD

#ifdef __HIPCC__
namespace bsdc_internal {  // csrc/bsdc_kernels.hip: the context's device and error text
int ctx_device(const bsdc_ctx *c);
int32_t ctx_fail(bsdc_ctx *c, int32_t code, const std::string &msg);
}  // namespace bsdc_internal
#endif

namespace {

constexpr int kImgT = 256;       // threads per workgroup
constexpr int kImgLanes = 16;    // lanes per record
constexpr int kImgRecs = kImgT / kImgLanes;

struct ImgArgs {
    const uint8_t *raw;
    int64_t n_raw;
    const bsdc_image_rec *recs;
    int64_t n_rec;
    int64_t n_slots;
    uint8_t *seq, *qual;
};

// 0, or which field of the entry is out of range: 1 src, 2 skip + len, 3 slot % 4, 4 slot
BSDC_HD int img_rec_check(const bsdc_image_rec &r, int64_t n_raw, int64_t n_slots) {
    if (r.src < 0 || r.l_seq < 0 || r.src > n_raw || ((int64_t)r.l_seq + 1) / 2 + r.l_seq > n_raw - r.src) return 1;
    if (r.skip < 0 || r.len < 0 || (int64_t)r.skip + r.len > r.l_seq) return 2;
    if (r.slot & 3u) return 3;
    if ((int64_t)r.slot + 1 + r.len > n_slots) return 4;
    return 0;
}

// aligned dword a of raw, little-endian; bytes outside [0, n_raw) read as 0
BSDC_HD uint32_t img_ld(const uint8_t *raw, int64_t n_raw, int64_t a) {
    const int64_t o = 4 * a;
    if (a < 0 || o >= n_raw) return 0;
    if (o + 4 <= n_raw) return *reinterpret_cast<const uint32_t *>(raw + o);
    uint32_t v = 0;
    for (int b = 0; o + b < n_raw; b++) v |= (uint32_t)raw[o + b] << (8 * b);
    return v;
}

// dwords of the qual image / the packed image that hold bases of the record
BSDC_HD int64_t img_nq(const bsdc_image_rec &r) { return r.len > 0 ? r.len / 4 + 1 : 0; }
BSDC_HD int64_t img_ns(const bsdc_image_rec &r) {
    return r.len > 0 ? (((int64_t)r.slot + r.len) >> 3) - ((int64_t)r.slot >> 3) + 1 : 0;
}

// qual dword k of the record: image bytes slot + 4k .. slot + 4k + 3, byte b = qual 4k + b - 1
BSDC_HD void img_qual(const ImgArgs &A, const bsdc_image_rec &r, int64_t k) {
    const int64_t D = ((int64_t)r.slot >> 2) + k;
    if (D >= (A.n_slots >> 2)) return;
    const int64_t P = r.src + ((int64_t)r.l_seq + 1) / 2 + r.skip + 4 * k - 1;  // source byte of image byte 4D
    const int64_t a = P >> 2;
    const int sh = (int)(P & 3) * 8;
    uint32_t x = img_ld(A.raw, A.n_raw, a);
    if (sh) x = (x >> sh) | (img_ld(A.raw, A.n_raw, a + 1) << (32 - sh));
    const int lo = k == 0 ? 1 : 0;
    const int64_t left = (int64_t)r.len + 1 - 4 * k;  // image bytes from 4D to the last qual's
    uint32_t m = 0xFFFFFFFFu << (8 * lo);
    if (left < 4) m &= (1u << (8 * (int)left)) - 1u;
    reinterpret_cast<uint32_t *>(A.qual)[D] = x & m;
}

// seq dword k of the record: image nibbles 8D .. 8D + 7 (D = slot / 8 + k), nibble n = base
// 8D + n - slot - 1; stored whole when both 4-nibble halves lie in the record's slot
BSDC_HD void img_seq(const ImgArgs &A, const bsdc_image_rec &r, int64_t k) {
    const int64_t S = r.slot, D = (S >> 3) + k;
    if (D >= (A.n_slots >> 3)) return;
    const int64_t P = 2 * r.src + r.skip + 8 * D - S - 1;  // source nibble of image nibble 8D
    const int64_t a = P >> 3;
    const int sh = (int)(P & 7) * 4;
    uint32_t v = __builtin_bswap32(img_ld(A.raw, A.n_raw, a));  // the first nibble on top
    if (sh) v = (v << sh) | (__builtin_bswap32(img_ld(A.raw, A.n_raw, a + 1)) >> (32 - sh));
    const int64_t lo = S + 1 - 8 * D;           // 1 or 5 in the record's first dword, else <= 0
    const int64_t hi = S + 1 + r.len - 8 * D;   // > 0: nibbles of the dword up to the last base's
    uint32_t m = lo > 0 ? 0xFFFFFFFFu >> (4 * (int)lo) : 0xFFFFFFFFu;
    if (hi < 8) m &= ~(0xFFFFFFFFu >> (4 * (int)hi));
    const uint32_t out = __builtin_bswap32(v & m);
    const int64_t cap = ((int64_t)r.len + 2 + 3) & ~(int64_t)3;
    const bool h0 = 8 * D >= S, h1 = 8 * D + 8 <= S + cap;
    if (h0 && h1)
        reinterpret_cast<uint32_t *>(A.seq)[D] = out;
    else if (h0)
        reinterpret_cast<uint16_t *>(A.seq)[2 * D] = (uint16_t)out;
    else if (h1)
        reinterpret_cast<uint16_t *>(A.seq)[2 * D + 1] = (uint16_t)(out >> 16);
}

// item t of the record: its qual dwords, then its seq dwords
BSDC_HD void img_item(const ImgArgs &A, const bsdc_image_rec &r, int64_t t, int64_t nq) {
    if (t < nq)
        img_qual(A, r, t);
    else
        img_seq(A, r, t - nq);
}

thread_local std::string g_img_err;

int32_t img_fail(bsdc_ctx *c, const std::string &m) {
    g_img_err = m;
#ifdef __HIPCC__
    if (c) bsdc_internal::ctx_fail(c, BSDC_EINVAL, m);
#else
    (void)c;
#endif
    return BSDC_EINVAL;
}

// the arguments and the whole table, as the launcher and the twin both refuse them
int32_t img_check(bsdc_ctx *c, const char *who, const uint8_t *raw, int64_t n_raw, const bsdc_image_rec *recs,
                  int64_t n_rec, int64_t n_slots, const uint8_t *seq_img, const uint8_t *qual_img) {
    const std::string w(who);
    if (n_raw < 0 || n_rec < 0 || n_slots < 0 || (n_raw > 0 && !raw) || (n_rec > 0 && !recs) || !seq_img || !qual_img)
        return img_fail(c, w + ": null pointer or negative count");
    if (n_slots & 7) return img_fail(c, w + ": n_slots must be a multiple of 8");
    if (((uintptr_t)raw & 3u) || ((uintptr_t)seq_img & 3u) || ((uintptr_t)qual_img & 3u) || ((uintptr_t)recs & 7u))
        return img_fail(c, w + ": raw, seq_img and qual_img must be 4-byte aligned, recs 8-byte aligned");
    static const char *const what[5] = {"", "src: the record's SEQ and QUAL bytes leave raw[0, n_raw)",
                                        "skip + len exceeds l_seq (or a negative skip / len)",
                                        "slot is not a multiple of 4", "slot + 1 + len exceeds n_slots"};
    for (int64_t i = 0; i < n_rec; i++)
        if (const int e = img_rec_check(recs[i], n_raw, n_slots))
            return img_fail(c, w + ": record " + std::to_string(i) + ": " + what[e]);
    return 0;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kImgT) void k_image_gather(ImgArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kImgRecs + (threadIdx.x / kImgLanes);
    if (i >= A.n_rec) return;
    const bsdc_image_rec r = A.recs[i];
    if (img_rec_check(r, A.n_raw, A.n_slots)) return;
    const int64_t nq = img_nq(r), n = nq + img_ns(r);
    for (int64_t t = threadIdx.x % kImgLanes; t < n; t += kImgLanes) img_item(A, r, t, nq);
}
#endif

}  // namespace

extern "C" {

const char *bsdc_image_last_error(void) { return g_img_err.c_str(); }

int32_t bsdc_image_gather_host(bsdc_ctx *ctx, const uint8_t *raw, int64_t n_raw, const bsdc_image_rec *recs,
                               int64_t n_rec, int64_t n_slots, uint8_t *seq_img, uint8_t *qual_img) {
    if (const int32_t rc = img_check(ctx, "bsdc_image_gather_host", raw, n_raw, recs, n_rec, n_slots, seq_img, qual_img))
        return rc;
    memset(seq_img, 0, (size_t)(n_slots / 2));
    memset(qual_img, 0, (size_t)n_slots);
    const ImgArgs A = {raw, n_raw, recs, n_rec, n_slots, seq_img, qual_img};
    for (int64_t i = 0; i < n_rec; i++) {
        const bsdc_image_rec r = recs[i];
        const int64_t nq = img_nq(r), n = nq + img_ns(r);
        for (int64_t t = 0; t < n; t++) img_item(A, r, t, nq);
    }
    return 0;
}

#ifdef __HIPCC__
int32_t bsdc_image_gather(bsdc_ctx *ctx, const uint8_t *raw, int64_t n_raw, const bsdc_image_rec *recs,
                          const bsdc_image_rec *recs_host, int64_t n_rec, int64_t n_slots, uint8_t *seq_img,
                          uint8_t *qual_img, void *stream) {
    if (!ctx) return img_fail(nullptr, "bsdc_image_gather: null context");
    if (n_rec > 0 && !recs_host) return img_fail(ctx, "bsdc_image_gather: recs_host (the table's host copy) is null");
    if (n_rec > (int64_t)0x7FFFFFFF * kImgRecs) return img_fail(ctx, "bsdc_image_gather: too many records for one launch");
    // (the host copy is what gets checked; recs only has to be non-null and aligned)
    if (const int32_t rc = img_check(ctx, "bsdc_image_gather", raw, n_raw, recs_host, n_rec, n_slots, seq_img, qual_img))
        return rc;
    if ((n_rec > 0 && !recs) || ((uintptr_t)recs & 7u)) return img_fail(ctx, "bsdc_image_gather: recs null or not 8-byte aligned");
    hipError_t e = hipSetDevice(bsdc_internal::ctx_device(ctx));
    if (e != hipSuccess) return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipStream_t st = (hipStream_t)stream;
    if (n_slots) {
        e = hipMemsetAsync(seq_img, 0, (size_t)(n_slots / 2), st);
        if (e == hipSuccess) e = hipMemsetAsync(qual_img, 0, (size_t)n_slots, st);
        if (e != hipSuccess) return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("image memset: ") + hipGetErrorString(e));
    }
    if (n_rec) {
        const ImgArgs A = {raw, n_raw, recs, n_rec, n_slots, seq_img, qual_img};
        hipLaunchKernelGGL(k_image_gather, dim3((unsigned)((n_rec + kImgRecs - 1) / kImgRecs)), dim3(kImgT), 0, st, A);
        e = hipGetLastError();
        if (e != hipSuccess)
            return bsdc_internal::ctx_fail(ctx, BSDC_EDEVICE, std::string("k_image_gather launch: ") + hipGetErrorString(e));
    }
    return 0;
}
#endif

}  // extern "C"
