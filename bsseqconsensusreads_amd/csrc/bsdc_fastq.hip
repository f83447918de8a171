// FASTQ emission on the GPU (gfx950): the text of a batch's kept families formatted from the
// consensus where the vote (and the filter) left it in HBM, and the CRC32 of every 65280-byte BGZF
// block of that text, so that with bsdc_bgzf.hip's deflate only compressed blocks cross PCIe
// (include/bsdc.h).  The bytes are those of libbsdc_io's format_fastq for
// forward records (picard SamToFastq's, main.snake.py:58-67,167-177).
//
// bsdc_fastq_format, three launches and the text on one stream, no host step between them:
//  1-3. the offset scan of bsdc_devtext.h (k_scan_sum / k_scan_scan / k_scan_off, shared with
//     bsdc_bam.hip) over the families' byte counts per file -> off[d][f], off[d][n_fam] = the total;
//  4. k_fq_text: one wavefront per (family, end).  A record starts at any byte of the text, so a
//     lane owns one ALIGNED dword of the destination at a time (bsdc_devtext.h store_record): it
//     assembles the dword's four bytes in a register and stores it whole; only a record's first
//     and last partial dword (and a dword that would cross `cap`) leave as single bytes.  A dword
//     inside SEQ takes its four nt16 codes from two or three packed bytes and maps them through a
//     16-byte register table with v_perm_b32; a dword inside QUAL is an unaligned dword of the
//     quality row (load4: two aligned loads, funnel shift) plus 33 in every byte, no carry between
//     bytes; the name, the separators and the seams go byte by byte.
// bsdc_bgzf_crc32: one 256-thread workgroup per block.  The block is staged in LDS (16-byte
// loads), thread t runs the raw CRC (register 0, no final xor) over segment t of 255 bytes by
// slice-by-4 (tables in LDS, 4 KB), multiplies it by x^(8 * 255 * (255 - t)) mod P -- the raw CRC
// is linear, so that is the segment's CRC followed by the zero bytes of the segments after it --
// and the 256 products are xor-ed; the 0xFFFFFFFF register start and final xor of a 65280-byte
// message are one constant.  Tables, powers and the constant are computed at compile time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bsdc.h"
#include "bsdc_devtext.h"

namespace {

using namespace bsdc_devtext;  // kT, kFamPerGroup, nt16x4, load4, store_record, the scan

constexpr int kSeg = 255;  // bytes per thread segment of a BGZF block (bsdc_bgzf.hip's segmentation)
constexpr int kBlock = kT * kSeg;
constexpr int kMaxName = 254;
constexpr uint32_t kPoly = 0xEDB88320u;  // the gzip polynomial, reflected: bit 31 is x^0

// a * b mod P (reflected representation)
constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

struct CrcTables {
    uint32_t t[4][256];  // slice-by-4
    uint32_t xn[256];    // x^(8 * kSeg * (255 - t)) mod P: the bytes after segment t
    uint32_t k;          // crc32 of kBlock zero bytes: what the register start and the final xor add
};

constexpr CrcTables make_crc_tables() {
    CrcTables T{};
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int j = 0; j < 8; j++) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
        T.t[0][n] = c;
    }
    for (int s = 1; s < 4; s++)
        for (uint32_t n = 0; n < 256; n++) T.t[s][n] = T.t[0][T.t[s - 1][n] & 0xffu] ^ (T.t[s - 1][n] >> 8);
    uint32_t seg = 0x80000000u, sq = 0x00800000u;  // x^(8 * kSeg) by square and multiply from x^8
    for (int e = kSeg; e; e >>= 1) {
        if (e & 1) seg = mulmod(seg, sq);
        sq = mulmod(sq, sq);
    }
    T.xn[255] = 0x80000000u;
    for (int t = 254; t >= 0; t--) T.xn[t] = mulmod(T.xn[t + 1], seg);
    T.k = mulmod(mulmod(T.xn[0], seg), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    return T;
}

__constant__ CrcTables cCrc = make_crc_tables();

// the raw CRC of p[0, n) from register c; t = the slice-by-4 tables; dwords are read where p + i is
// 4-byte aligned
BSDC_HD uint32_t crc_raw(const uint32_t (*t)[256], const uint8_t *p, int n, uint32_t c) {
    int i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 3u); i++) c = t[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    for (; i + 4 <= n; i += 4) {
        c ^= *reinterpret_cast<const uint32_t *>(p + i);
        c = t[3][c & 0xffu] ^ t[2][(c >> 8) & 0xffu] ^ t[1][(c >> 16) & 0xffu] ^ t[0][c >> 24];
    }
    for (; i < n; i++) c = t[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

struct CrcSmem {
    uint32_t t[4][256];
    uint32_t part[kT / 64];
    alignas(16) uint8_t data[kBlock];
};

__global__ __launch_bounds__(kT) void k_crc32(const uint8_t *__restrict__ in, int64_t blk0, uint32_t *__restrict__ crc) {
    __shared__ CrcSmem S;
    const int tid = threadIdx.x;
    const int64_t blk = blk0 + blockIdx.x;
    for (int s = 0; s < 4; s++) S.t[s][tid] = cCrc.t[s][tid];
    const uint4 *src = reinterpret_cast<const uint4 *>(in + blk * kBlock);
    uint4 *dst = reinterpret_cast<uint4 *>(S.data);
    for (int i = tid; i < kBlock / 16; i += kT) dst[i] = src[i];
    __syncthreads();
    uint32_t c = crc_raw(S.t, S.data + tid * kSeg, kSeg, 0u);
    c = mulmod(cCrc.xn[tid], c);
    for (int o = 32; o; o >>= 1) c ^= __shfl_xor(c, o);
    if ((tid & 63) == 0) S.part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) crc[blk] = S.part[0] ^ S.part[1] ^ S.part[2] ^ S.part[3] ^ cCrc.k;
}

// ---- the FASTQ text ----

struct FqArgs {
    const uint8_t *status;
    const uint16_t *len;
    const uint8_t *seq;
    const uint8_t *qual;
    const uint8_t *filt;
    const int64_t *name_off;
    const uint8_t *name_buf;
    int64_t n_fam;
    int32_t stride;
    int64_t *off[2];
    uint8_t *text[2];
    int64_t cap[2];
    int64_t *bsum;  // [2][groups + 1]
    int64_t groups;
};

BSDC_HD bool fq_kept(const FqArgs &A, int64_t f) { return (A.status[f] & 1) && (A.filt == nullptr || A.filt[f] == 0); }
BSDC_HD int fq_len(const FqArgs &A, int64_t f, int d) {
    const int l = A.len[2 * f + d];
    return l < A.stride ? l : A.stride;  // (a row holds stride bases: no read past it whatever len says)
}
BSDC_HD int fq_name_len(const FqArgs &A, int64_t f) {
    const int64_t n = A.name_off[f + 1] - A.name_off[f];
    return n < 0 ? 0 : n > kMaxName ? kMaxName : (int)n;  // (the host checked its copy: 0..254)
}
// bytes of family f in file d: '@' name '/' N '\n' SEQ '\n' '+' '\n' QUAL '\n'
BSDC_HD int64_t fq_bytes(const FqArgs &A, int64_t f, int d) {
    return fq_kept(A, f) ? 8 + fq_name_len(A, f) + 2 * fq_len(A, f, d) : 0;
}

// One record (family f, end d): name nm[0, nl), packed bases sq, qualities ql, L bases.
struct FqRec {
    const uint8_t *nm, *sq, *ql;
    int nl, L, d, size;
};

// byte i of the record (0 outside it)
BSDC_HD uint32_t fq_byte(const FqRec &r, int i) {
    if (i < 0 || i >= r.size) return 0;
    if (i == 0) return '@';
    if (i <= r.nl) return r.nm[i - 1];
    i -= r.nl + 1;
    if (i == 0) return '/';
    if (i == 1) return (uint32_t)('1' + r.d);
    if (i == 2) return '\n';
    i -= 3;
    if (i < r.L) {
        const uint32_t b = r.sq[i >> 1];
        return nt16x4((i & 1) ? (b & 15u) : (b >> 4)) & 0xffu;
    }
    i -= r.L;
    if (i == 0 || i == 2) return '\n';
    if (i == 1) return '+';
    i -= 3;
    if (i < r.L) return (uint32_t)(uint8_t)(33 + r.ql[i]);
    return '\n';
}

// bytes i0 .. i0 + 3 of the record as one little-endian dword (bytes outside the record: 0)
BSDC_HD uint32_t fq_dword(const FqRec &r, int i0) {
    const int s0 = r.nl + 4, q0 = r.nl + 7 + r.L;
    // inside QUAL: an unaligned dword of the row (its second aligned dword holds a byte of the four), + 33 per byte
    if (i0 >= q0 && i0 + 4 <= q0 + r.L) return add33x4(load4(r.ql + (i0 - q0)));
    if (i0 >= s0 && i0 + 4 <= s0 + r.L) {  // inside SEQ: codes j .. j + 3 of the packed row, high nibble first
        const int j = i0 - s0, s = j & 1;
        const uint8_t *a = r.sq + (j >> 1);
        const uint32_t W = (uint32_t)a[0] << 16 | (uint32_t)a[1] << 8 | (s ? (uint32_t)a[2] : 0u);
        const uint32_t c = ((W >> (20 - 4 * s)) & 15u) | ((W >> (16 - 4 * s)) & 15u) << 8 |
                           ((W >> (12 - 4 * s)) & 15u) << 16 | ((W >> (8 - 4 * s)) & 15u) << 24;
        return nt16x4(c);
    }
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) v |= fq_byte(r, i0 + b) << (8 * b);
    return v;
}

BSDC_HD FqRec fq_rec(const FqArgs &A, int64_t f, int d) {
    FqRec r;
    r.nm = A.name_buf + A.name_off[f];
    r.sq = A.seq + (2 * f + d) * (int64_t)(A.stride / 2);
    r.ql = A.qual + (2 * f + d) * (int64_t)A.stride;
    r.nl = fq_name_len(A, f);
    r.L = fq_len(A, f, d);
    r.d = d;
    r.size = 8 + r.nl + 2 * r.L;
    return r;
}

BSDC_HD int64_t scan_bytes(const FqArgs &A, int64_t f, int d) { return fq_bytes(A, f, d); }
BSDC_HD int64_t *scan_off(const FqArgs &A, int d) { return A.off[d]; }

__global__ __launch_bounds__(kT) void k_fq_text(FqArgs A) {
    const int64_t w = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int64_t f = w >> 1;
    const int d = (int)(w & 1);
    if (f >= A.n_fam || !fq_kept(A, f)) return;
    const FqRec r = fq_rec(A, f, d);
    store_record(A.text[d], A.off[d][f], r.size, A.cap[d], threadIdx.x & 63, 64, [r](int i0) { return fq_dword(r, i0); });
}

}  // namespace

extern "C" {

int64_t bsdc_fastq_text_bound(int64_t n_fam, int64_t name_bytes, int32_t stride) {
    if (n_fam < 0 || name_bytes < 0 || stride < 0) return -1;
    return 8 * n_fam + name_bytes + 2 * n_fam * (int64_t)stride;
}

int64_t bsdc_fastq_tmp_bytes(int64_t n_fam) {
    if (n_fam < 0) return -1;
    return 2 * ((n_fam + kFamPerGroup - 1) / kFamPerGroup + 1) * (int64_t)sizeof(int64_t);
}

int32_t bsdc_fastq_format(const bsdc_consensus *out, const uint8_t *filt, int64_t n_fam, const int64_t *name_off,
                          const uint8_t *name_buf, const int64_t *name_off_host, int64_t *off0, int64_t *off1,
                          uint8_t *text0, uint8_t *text1, int64_t cap0, int64_t cap1, uint8_t *tmp, void *stream) {
    if (!out || !out->status || !out->len || !out->seq || !out->qual || !name_off || !name_buf || !name_off_host ||
        !off0 || !off1 || !text0 || !text1 || !tmp)
        return BSDC_EINVAL;
    if (n_fam < 0 || n_fam > (int64_t)1 << 30 || cap0 < 0 || cap1 < 0 || out->stride <= 0 || out->stride % 16 != 0)
        return BSDC_EINVAL;
    if (((uintptr_t)out->qual & 3u) || ((uintptr_t)tmp & 7u) || ((uintptr_t)off0 & 7u) || ((uintptr_t)off1 & 7u))
        return BSDC_EINVAL;
    for (int64_t f = 0; f < n_fam; f++) {
        const int64_t nl = name_off_host[f + 1] - name_off_host[f];
        if (nl < 0 || nl > kMaxName) return BSDC_EINVAL;
    }
    FqArgs A;
    A.status = out->status;
    A.len = out->len;
    A.seq = out->seq;
    A.qual = out->qual;
    A.filt = filt;
    A.name_off = name_off;
    A.name_buf = name_buf;
    A.n_fam = n_fam;
    A.stride = out->stride;
    A.off[0] = off0;
    A.off[1] = off1;
    A.text[0] = text0;
    A.text[1] = text1;
    A.cap[0] = cap0;
    A.cap[1] = cap1;
    A.bsum = reinterpret_cast<int64_t *>(tmp);
    A.groups = (n_fam + kFamPerGroup - 1) / kFamPerGroup;
    hipStream_t st = (hipStream_t)stream;
    launch_scan<2>(A, st);
    if (A.groups) {
        const int64_t waves = 2 * n_fam;
        hipLaunchKernelGGL(k_fq_text, dim3((unsigned)((waves + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, A);
    }
    return hipGetLastError() == hipSuccess ? 0 : BSDC_EDEVICE;
}

int32_t bsdc_bgzf_crc32(const uint8_t *in, int64_t blk0, int64_t nblk, uint32_t *crc, void *stream) {
    if (!in || !crc || blk0 < 0 || nblk < 0 || nblk > 0x7fffffff || ((uintptr_t)in & 15u) || ((uintptr_t)crc & 3u))
        return BSDC_EINVAL;
    if (nblk == 0) return 0;
    hipLaunchKernelGGL(k_crc32, dim3((unsigned)nblk), dim3(kT), 0, (hipStream_t)stream, in, blk0, crc);
    return hipGetLastError() == hipSuccess ? 0 : BSDC_EDEVICE;
}

}  // extern "C"
