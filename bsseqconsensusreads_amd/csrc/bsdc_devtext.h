// What the passes over the vote's outputs share (bsdc_fastq.hip, bsdc_bam.hip, bsdc_toolrec.hip,
// bsdc_zipper.hip; the macro also bsdc_image.hip, bsdc_metrics.hip, bsdc_filter.hip and
// bsdc_ssrows.h).  Everything here is a template or inline: each including file instantiates its
// own copy.
//
// The upper half is plain C++ and compiles under g++ (the host twins and libbsdc_io include it):
// BSDC_HD, the dword helpers and the "a lane owns one aligned destination dword" record writer.
// The lower half is hipcc's alone: the 64-lane wave reductions and the three-launch offset scan.
//
// The scan, over an argument record A of the including file (passed by value to the kernels):
//   A.n_fam, A.groups = ceil(n_fam / kFamPerGroup), A.bsum [D][groups + 1] int64 scratch,
//   scan_bytes(A, f, d) -> the bytes of family f in output d, scan_off(A, d) -> int64 [n_fam + 1].
//  1. k_scan_sum<D>: a workgroup sums the byte counts of its 1024 families, per output;
//  2. k_scan_scan<D>: one workgroup scans the workgroups' sums in place (tiles of 256 with a carry)
//     and writes the totals to off[d][n_fam];
//  3. k_scan_off<D>: each workgroup scans its families' counts again from its base -> off[d][f].
#ifndef BSDC_DEVTEXT_H
#define BSDC_DEVTEXT_H
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BSDC_HD __host__ __device__ __forceinline__
#else
#define BSDC_HD inline
#endif

namespace bsdc_devtext {

constexpr int kT = 256;  // threads per workgroup
constexpr int kFamPerThread = 4;
constexpr int kFamPerGroup = kT * kFamPerThread;

// four nt16 codes (one per byte, 0..15) -> their letters of "=ACMGRSVTWYHKDBN"
BSDC_HD uint32_t nt16x4(uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first
    const uint32_t sel = c & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(0x56535247u /* GRSV */, 0x4D43413Du /* =ACM */, sel);
    const uint32_t hi = __builtin_amdgcn_perm(0x4E42444Bu /* KDBN */, 0x48595754u /* TWYH */, sel);
    const uint32_t m = ((c >> 3) & 0x01010101u) * 0xffu;
    return (lo & ~m) | (hi & m);
#else
    const char *t = "=ACMGRSVTWYHKDBN";
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) v |= (uint32_t)(uint8_t)t[(c >> (8 * b)) & 15u] << (8 * b);
    return v;
#endif
}

// + 33 in every byte, no carry between bytes ((uint8_t)(q + 33) four times)
BSDC_HD uint32_t add33x4(uint32_t x) { return ((x & 0x7f7f7f7fu) + 0x21212121u) ^ (x & 0x80808080u); }

// bytes a[0..3] as one little-endian dword by two aligned loads and a funnel shift.  The aligned
// dwords that hold a[0] and a[3] are read: the caller keeps both inside the source buffer (can4, or
// a row that starts 4-byte aligned, is a multiple of 4 long and holds a[0..3]).
BSDC_HD uint32_t load4(const uint8_t *a) {
    const int sh = (int)((uintptr_t)a & 3u);
    uint32_t x, y;
    memcpy(&x, __builtin_assume_aligned(a - sh, 4), 4);
    if (!sh) return x;
    memcpy(&y, __builtin_assume_aligned(a - sh + 4, 4), 4);
    return (x >> (8 * sh)) | (y << (32 - 8 * sh));
}
// a[0..3] is inside [buf, buf + n) with the aligned dwords that hold a[0] and a[3] (buf 4-byte aligned)
BSDC_HD bool can4(const uint8_t *buf, int64_t n, const uint8_t *a) {
    return a >= buf && (int64_t)((a + 3 - buf) | 3) < n;
}

// The record writer: a record of `size` bytes starts at base + o, at any byte, and `cap` bytes of
// base are writable.  A lane (lane, lane + nlanes, ..) owns one ALIGNED dword of the destination at
// a time: dword k covers the record's bytes i0 = 4k - ho .., ho = the start's offset in its dword;
// dword_of(i0) gives bytes i0 .. i0 + 3 of the record (whatever it likes outside [0, size)).  A
// dword inside the record and below cap is stored whole, else the bytes inside both.
template <class F>
BSDC_HD void store_record(uint8_t *base, int64_t o, int size, int64_t cap, int lane, int nlanes, F dword_of) {
    const int ho = (int)((uintptr_t)(base + o) & 3u);
    const int nd = (ho + size + 3) >> 2;
    for (int k = lane; k < nd; k += nlanes) {
        const int i0 = 4 * k - ho;
        const uint32_t v = dword_of(i0);
        const int64_t p = o + i0;
        if (i0 >= 0 && i0 + 4 <= size && p + 4 <= cap) {
            memcpy(__builtin_assume_aligned(base + p, 4), &v, 4);  // (aligned: one dword store)
            continue;
        }
        for (int b = 0; b < 4; b++)
            if (i0 + b >= 0 && i0 + b < size && p + b < cap) base[p + b] = (uint8_t)(v >> (8 * b));
    }
}

#ifdef __HIPCC__
// wave reductions (64 lanes): every lane gets the result
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) { return (int64_t)wave_sum((uint64_t)v); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor((int)v, m, 64);
        v = x > v ? x : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor((int)v, m, 64);
        v = x < v ? x : v;
    }
    return v;
}

// exclusive scan of one value per thread over the workgroup (sh: 2 * kT values); *total = the sum
__device__ __forceinline__ int64_t group_scan(int64_t v, int64_t *sh, int64_t *total) {
    const int t = threadIdx.x;
    int cur = 0;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kT; o <<= 1) {
        int64_t x = sh[cur * kT + t];
        if (t >= o) x += sh[cur * kT + t - o];
        cur ^= 1;
        sh[cur * kT + t] = x;
        __syncthreads();
    }
    const int64_t inc = sh[cur * kT + t];
    *total = sh[cur * kT + kT - 1];
    __syncthreads();
    return inc - v;
}

template <int D, class Args>
__global__ __launch_bounds__(kT) void k_scan_sum(Args A) {
    __shared__ int64_t sh[2 * kT];
    const int64_t f0 = (int64_t)blockIdx.x * kFamPerGroup + threadIdx.x * kFamPerThread;
    for (int d = 0; d < D; d++) {
        int64_t s = 0, total;
        for (int j = 0; j < kFamPerThread; j++)
            if (f0 + j < A.n_fam) s += scan_bytes(A, f0 + j, d);
        group_scan(s, sh, &total);
        if (threadIdx.x == 0) A.bsum[d * (A.groups + 1) + blockIdx.x] = total;
    }
}

template <int D, class Args>
__global__ __launch_bounds__(kT) void k_scan_scan(Args A) {
    __shared__ int64_t sh[2 * kT];
    for (int d = 0; d < D; d++) {
        int64_t *b = A.bsum + d * (A.groups + 1);
        int64_t carry = 0;
        for (int64_t g0 = 0; g0 < A.groups; g0 += kT) {
            const int64_t g = g0 + threadIdx.x;
            const int64_t v = g < A.groups ? b[g] : 0;
            int64_t total;
            const int64_t ex = group_scan(v, sh, &total);
            if (g < A.groups) b[g] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) scan_off(A, d)[A.n_fam] = carry;
    }
}

template <int D, class Args>
__global__ __launch_bounds__(kT) void k_scan_off(Args A) {
    __shared__ int64_t sh[2 * kT];
    const int64_t f0 = (int64_t)blockIdx.x * kFamPerGroup + threadIdx.x * kFamPerThread;
    for (int d = 0; d < D; d++) {
        int64_t n[kFamPerThread], s = 0, total;
        for (int j = 0; j < kFamPerThread; j++) {
            n[j] = f0 + j < A.n_fam ? scan_bytes(A, f0 + j, d) : 0;
            s += n[j];
        }
        int64_t o = A.bsum[d * (A.groups + 1) + blockIdx.x] + group_scan(s, sh, &total);
        int64_t *off = scan_off(A, d);
        for (int j = 0; j < kFamPerThread; j++) {
            if (f0 + j < A.n_fam) off[f0 + j] = o;
            o += n[j];
        }
    }
}

// the three launches on `st` (nothing when there is no family but the totals)
template <int D, class Args>
inline void launch_scan(const Args &A, hipStream_t st) {
    if (A.groups) hipLaunchKernelGGL((k_scan_sum<D, Args>), dim3((unsigned)A.groups), dim3(kT), 0, st, A);
    hipLaunchKernelGGL((k_scan_scan<D, Args>), dim3(1), dim3(kT), 0, st, A);
    if (A.groups) hipLaunchKernelGGL((k_scan_off<D, Args>), dim3((unsigned)A.groups), dim3(kT), 0, st, A);
}

#endif  // __HIPCC__

}  // namespace bsdc_devtext
#endif
