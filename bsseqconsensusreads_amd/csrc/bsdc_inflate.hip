// BGZF block inflate on the GPU (gfx950): one 64-thread workgroup (one wave) per BGZF block of the
// input BAM -> the block's bytes (RFC 1951 raw DEFLATE, any number of stored / fixed / dynamic
// deflate blocks per BGZF block).  The host checks CRC32 and ISIZE on the returned bytes
// (libbsdc_io inflate_blocks); no CRC here.
//
// The input is untrusted.  Everything that reads the compressed bits or decides a copy is in the
// __host__ __device__ functions of namespace inf below, which the kernel and the sequential host
// twin bsdc_bgzf_inflate_host both run (lane 0 of 1 on the host), so every corrupt input the GPU
// tests use has first gone through the same functions on the CPU between guard bytes
// (tests/test_inflate_host.py):
//  - the bit reader returns zeros past the block's clen bytes and says so (over());
//  - the output window lives in LDS (65536 bytes); a literal or a match is emitted only after
//    outpos + length <= isize and distance <= outpos held, so a copy neither leaves the window nor
//    reads its own unwritten bytes; the window goes to `out` only when the block ended with
//    exactly isize bytes (an erroneous block writes nothing);
//  - every round of the block loop consumes at least one input bit or ends the block, and a
//    reader past its end is an error, so the loop ends on any bytes.
//
// Rounds (the workgroup alternates them until BFINAL's end of block):
//  H. header: the wave loads the next 2 KiB of compressed bytes into LDS (aligned dwords); lane 0
//     reads BFINAL/BTYPE and, for a dynamic block, the code-length code and the HLIT + HDIST
//     lengths (repeat codes 16/17/18 across the HLIT/HDIST boundary, as zlib).  The wave then
//     builds the literal/length and the distance decoders: lengths counted across lanes (LDS
//     atomics), zlib's over-subscribed / incomplete rules on the counts, canonical first codes,
//     every lane ranking and placing its symbols, and a 9-bit first-level table (entry = symbol
//     << 4 | length) filled across lanes; longer codes decode canonically behind it.  A stored
//     block is copied from `comp` by the wave.
//  T. tokens: the wave reloads the compressed window; lane 0 decodes up to 256 symbols into a
//     token ring (literal, or length / distance, with its output position); the wave writes the
//     ring's literals in parallel, then each match in order, 64 bytes a step: a non-overlapping
//     match as a plain copy, an overlapping one (distance < length) from its period (source byte
//     i mod distance).
//  W. write-out: the window to out + dst, 16-byte stores (the window sits in LDS at dst's
//     misalignment, so both sides are aligned), bytes at the two ends.
// Symbol decode is on one lane per block (the first version the design allows);
// the table build, the copies and the write-out are wave-wide.  LDS: 65552 window + 2048
// compressed + 1536 ring + ~3.5 KB tables = 72.5 KB, two workgroups per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bsdc.h"

#define HD __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define INF_SYNC() __syncthreads()
#define INF_COUNT(p) atomicAdd((p), 1u)
#else
#define INF_SYNC() (void)0
#define INF_COUNT(p) (void)(*(p) += 1u)
#endif

namespace inf {

constexpr int kWin = 65536;       // the largest BGZF ISIZE
constexpr int kMaxClen = 1 << 24; // a block's compressed bytes (bit positions stay in 32 bits)
constexpr int kTok = 256;         // tokens per round
constexpr int kCompWin = 2048;    // compressed bytes in LDS per round: 256 tokens of <= 48 bits, or one
                                  // dynamic header (<= 17 + 57 + 316 * 14 bits), + the dword alignment
constexpr int kFastBits = 9;

enum { PH_HEADER = 0, PH_TOKENS = 1, PH_DONE = 2 };
enum { KIND_STORED = 0, KIND_HUFF = 1 };

struct Huff {
    uint16_t fast[1 << kFastBits];  // low 9 stream bits -> symbol << 4 | code length (0: a longer code, or none)
    uint16_t sorted[288];           // symbols by (length, symbol)
    uint32_t count[16];             // codes per length
    uint16_t first[16];             // first canonical code of each length
    uint16_t offs[16];              // its place in sorted
};

struct State {
    int32_t bitpos, outpos, nt, err, phase, bfinal, kind;
    int32_t stored_from, stored_len, hlit, hdist;
};

struct Tables {
    Huff lit, dist;
    uint8_t lens[288 + 32];
    uint8_t clfast[128];  // the code-length code, 7 bits: symbol << 3 | length (0: none)
};

// LSB-first bit reader over the block's bytes [0, n): byte i is win[i - base] for base <= i <
// base + wlen (the kernel's LDS window; the host passes the whole block), zero at and past n.
struct Bits {
    const uint8_t *win;
    int32_t base, wlen, n;
    uint64_t buf;
    int32_t cnt, next;
    bool bad;  // a byte inside the block but outside the window was asked for (a round's budget was wrong)
    HD void start(const uint8_t *w, int32_t b, int32_t wl, int32_t nn, int32_t bitpos) {
        win = w;
        base = b;
        wlen = wl;
        n = nn;
        buf = 0;
        cnt = 0;
        next = bitpos >> 3;
        bad = false;
        fill();
        drop(bitpos & 7);
    }
    HD void fill() {
        while (cnt <= 48) {
            uint32_t b = 0;
            if (next < n) {
                const int32_t k = next - base;
                if (k >= 0 && k < wlen) b = win[k];
                else bad = true;
            }
            buf |= (uint64_t)b << cnt;
            cnt += 8;
            next++;
        }
    }
    HD uint32_t peek(int k) {  // k <= 16
        fill();
        return (uint32_t)buf & ((1u << k) - 1u);
    }
    HD void drop(int k) {
        buf >>= k;
        cnt -= k;
    }
    HD uint32_t get(int k) {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    HD int32_t bitpos() const { return next * 8 - cnt; }
    HD bool over() const { return bad || bitpos() > 8 * n; }  // consumed bits the block does not have
};

HD int fail(const Bits &br, int code) { return br.over() ? BSDC_INFLATE_EINPUT : code; }

// RFC 1951 3.2.5 as arithmetic
HD int len_base(int c) { return c < 8 ? c + 3 : c == 28 ? 258 : ((4 + (c & 3)) << ((c >> 2) - 1)) + 3; }
HD int len_extra(int c) { return c < 8 || c == 28 ? 0 : (c >> 2) - 1; }
HD int dist_base(int e) { return e < 4 ? e + 1 : ((2 + (e & 1)) << ((e >> 1) - 1)) + 1; }
HD int dist_extra(int e) { return e < 4 ? 0 : (e >> 1) - 1; }

// zlib inftrees.c's verdict on a set of code-length counts: over-subscribed never; incomplete only
// for the literal/length and distance codes when the longest code has one bit; no code at all is
// accepted (using it is the error).
HD bool counts_valid(const uint32_t *count, bool is_codelen_code) {
    int left = 1, mx = 0;
    for (int l = 1; l <= 15; l++) {
        left <<= 1;
        left -= (int)count[l];
        if (left < 0) return false;
        if (count[l]) mx = l;
    }
    if (mx == 0) return true;
    return !(left > 0 && (is_codelen_code || mx != 1));
}

// one symbol; -1: the bits are no code of this set
HD int decode(Bits &br, const Huff &h) {
    const uint32_t v = br.peek(15);
    const uint32_t e = h.fast[v & ((1u << kFastBits) - 1u)];
    if (e) {
        br.drop((int)(e & 15u));
        return (int)(e >> 4);
    }
    const uint32_t r = __builtin_bitreverse32(v) >> 17;  // the 15 bits, first stream bit highest
    for (int l = kFastBits + 1; l <= 15; l++) {
        const uint32_t d = (r >> (15 - l)) - h.first[l];
        if (d < h.count[l]) {
            br.drop(l);
            return h.sorted[h.offs[l] + d];
        }
    }
    return -1;
}

// The decoder of lens[0, n) by `nl` lanes (all call it; *err is the block's, in shared memory).
HD void huff_build(const uint8_t *lens, int n, Huff &h, int lane, int nl, int32_t *err) {
    for (int i = lane; i < 16; i += nl) h.count[i] = 0;
    for (int i = lane; i < (1 << kFastBits); i += nl) h.fast[i] = 0;
    INF_SYNC();
    for (int i = lane; i < n; i += nl)
        if (lens[i]) INF_COUNT(&h.count[lens[i]]);
    INF_SYNC();
    if (lane == 0) {
        if (!counts_valid(h.count, false) && !*err) *err = BSDC_INFLATE_ELENGTHS;
        uint32_t code = 0, o = 0;
        h.first[0] = h.offs[0] = 0;
        for (int l = 1; l <= 15; l++) {
            code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
            h.first[l] = (uint16_t)code;
            h.offs[l] = (uint16_t)o;
            o += h.count[l];
        }
    }
    INF_SYNC();
    if (*err) return;  // (uniform: every lane reads it after the barrier; an over-subscribed set would overrun fast[])
    for (int s = lane; s < n; s += nl) {
        const int l = lens[s];
        if (!l) continue;
        uint32_t rank = 0;
        for (int j = 0; j < s; j++) rank += lens[j] == l;
        h.sorted[h.offs[l] + rank] = (uint16_t)s;  // (offs + rank < the number of coded symbols <= n <= 288)
        if (l <= kFastBits) {
            const uint32_t code = h.first[l] + rank;  // < 1 << l: the counts are not over-subscribed
            const uint32_t rev = __builtin_bitreverse32(code) >> (32 - l);
            for (uint32_t k = rev; k < (1u << kFastBits); k += 1u << l) h.fast[k] = (uint16_t)(s << 4 | l);
        }
    }
    INF_SYNC();
}

// Round H on lane 0: the deflate block's header; for a dynamic block the HLIT + HDIST lengths into
// T.lens (distance lengths from T.lens + hlit), for a fixed block the fixed lengths.
HD void step_header(Bits &br, State &st, Tables &T) {
    st.bfinal = (int32_t)br.get(1);
    const int type = (int)br.get(2);
    if (br.over()) {
        st.err = BSDC_INFLATE_EINPUT;
        return;
    }
    if (type == 3) {
        st.err = BSDC_INFLATE_EBTYPE;
        return;
    }
    if (type == 0) {
        br.drop((8 - (br.bitpos() & 7)) & 7);
        const uint32_t len = br.get(16), nlen = br.get(16);
        if (br.over()) {
            st.err = BSDC_INFLATE_EINPUT;
            return;
        }
        if (len != (~nlen & 0xFFFFu)) {
            st.err = BSDC_INFLATE_ESTORED;
            return;
        }
        st.kind = KIND_STORED;
        st.stored_from = br.bitpos() >> 3;
        st.stored_len = (int32_t)len;
        return;
    }
    st.kind = KIND_HUFF;
    if (type == 1) {
        for (int i = 0; i < 288; i++) T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; i++) T.lens[288 + i] = 5;
        st.hlit = 288;  // (286, 287 and distances 30, 31 have codes; using one is the error)
        st.hdist = 32;
        st.bitpos = br.bitpos();
        return;
    }
    const int hlit = (int)br.get(5) + 257, hdist = (int)br.get(5) + 1, hclen = (int)br.get(4) + 4;
    if (hlit > 286 || hdist > 30) {
        st.err = fail(br, BSDC_INFLATE_ECOUNTS);
        return;
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    uint32_t count[16];
    for (int i = 0; i < 19; i++) cl[i] = 0;
    for (int i = 0; i < 16; i++) count[i] = 0;
    for (int i = 0; i < hclen; i++) cl[order[i]] = (uint8_t)br.get(3);
    for (int i = 0; i < 19; i++) count[cl[i]]++;
    count[0] = 0;
    if (!counts_valid(count, true)) {
        st.err = fail(br, BSDC_INFLATE_ELENGTHS);
        return;
    }
    for (int i = 0; i < 128; i++) T.clfast[i] = 0;
    {
        uint32_t code = 0;
        for (int l = 1; l <= 7; l++) {
            code = (code + (l > 1 ? count[l - 1] : 0u)) << 1;
            uint32_t c = code;
            for (int s = 0; s < 19; s++) {
                if (cl[s] != l) continue;
                const uint32_t rev = __builtin_bitreverse32(c) >> (32 - l);  // c < 1 << l (not over-subscribed)
                for (uint32_t k = rev; k < 128; k += 1u << l) T.clfast[k] = (uint8_t)(s << 3 | l);
                c++;
            }
        }
    }
    const int total = hlit + hdist;  // <= 316
    int have = 0;
    while (have < total) {
        const uint32_t e = T.clfast[br.peek(7)];
        if (!e) {
            st.err = fail(br, BSDC_INFLATE_ECODE);
            return;
        }
        br.drop((int)(e & 7u));
        const int s = (int)(e >> 3);
        if (s < 16) {
            T.lens[have++] = (uint8_t)s;
        } else {
            int rep, v = 0;
            if (s == 16) {
                if (have == 0) {
                    st.err = fail(br, BSDC_INFLATE_EREPEAT);
                    return;
                }
                v = T.lens[have - 1];
                rep = 3 + (int)br.get(2);
            } else if (s == 17) {
                rep = 3 + (int)br.get(3);
            } else {
                rep = 11 + (int)br.get(7);
            }
            if (have + rep > total) {
                st.err = fail(br, BSDC_INFLATE_EREPEAT);
                return;
            }
            while (rep-- > 0) T.lens[have++] = (uint8_t)v;
        }
        if (br.over()) {
            st.err = BSDC_INFLATE_EINPUT;
            return;
        }
    }
    if (T.lens[256] == 0) {
        st.err = BSDC_INFLATE_ENOEOB;
        return;
    }
    st.hlit = hlit;
    st.hdist = hdist;
    st.bitpos = br.bitpos();
}

// A stored block's copy, checked: its bytes lie inside the block and its output inside isize.
HD int stored_check(const State &st, int32_t n, int32_t isize) {
    if ((int64_t)st.stored_from + st.stored_len > n) return BSDC_INFLATE_EINPUT;
    if ((int64_t)st.outpos + st.stored_len > isize) return BSDC_INFLATE_EOVERFLOW;
    return 0;
}

// Round T on lane 0: up to kTok tokens, each checked against the bytes written so far and isize.
HD void step_tokens(Bits &br, State &st, const Tables &T, uint32_t *tok, uint16_t *tpos, int32_t isize) {
    int nt = 0;
    int32_t pos = st.outpos;
    while (nt < kTok) {
        const int s = decode(br, T.lit);
        int code = 0;
        if (s < 0) {
            code = BSDC_INFLATE_ECODE;
        } else if (s < 256) {
            if (pos >= isize) code = BSDC_INFLATE_EOVERFLOW;
            else {
                tok[nt] = (uint32_t)s;
                tpos[nt++] = (uint16_t)pos;
                pos++;
            }
        } else if (s == 256) {
            if (br.over()) code = BSDC_INFLATE_EINPUT;
            else st.phase = st.bfinal ? PH_DONE : PH_HEADER;
            if (!code) break;
        } else if (s > 285) {
            code = BSDC_INFLATE_ESYMBOL;
        } else {
            const int lc = s - 257;
            const int len = len_base(lc) + (int)br.get(len_extra(lc));
            const int ds = decode(br, T.dist);
            if (ds < 0) code = BSDC_INFLATE_ECODE;
            else if (ds >= 30) code = BSDC_INFLATE_ESYMBOL;
            else {
                const int d = dist_base(ds) + (int)br.get(dist_extra(ds));
                if (d > pos) code = BSDC_INFLATE_EDIST;
                else if (pos + len > isize) code = BSDC_INFLATE_EOVERFLOW;
                else {
                    tok[nt] = 0x80000000u | (uint32_t)len << 16 | (uint32_t)d;  // d <= 32768: 16 bits
                    tpos[nt++] = (uint16_t)pos;
                    pos += len;
                }
            }
        }
        if (code || br.over()) {
            st.err = fail(br, code ? code : BSDC_INFLATE_EINPUT);
            return;
        }
    }
    st.nt = nt;
    st.outpos = pos;
    st.bitpos = br.bitpos();
}

// A match of step_tokens (d <= p, p + len <= isize <= kWin) by nl lanes: byte i comes from the
// period, so a source is always below p (written, and by no lane of this copy).
HD void copy_match(uint8_t *w, int p, int len, int d, int lane, int nl) {
    for (int i0 = 0; i0 < len; i0 += nl) {
        const int i = i0 + lane;
        if (i < len) w[p + i] = w[p - d + (d >= len ? i : d == 1 ? 0 : i % d)];
    }
}

// A descriptor the block may be read and written through at all.
HD bool block_in_range(const bsdc_inflate_block &b, int64_t n_comp, int64_t n_out) {
    return b.src >= 0 && b.clen >= 0 && b.clen <= kMaxClen && b.src <= n_comp - b.clen && b.isize >= 0 &&
           b.isize <= kWin && b.dst >= 0 && b.dst <= n_out - b.isize;
}

struct __attribute__((aligned(16))) Work {
    uint8_t out[kWin + 16];
    alignas(16) uint8_t cw[kCompWin];
    Tables T;
    uint32_t tok[kTok];
    uint16_t tpos[kTok];
    State st;
};

#if defined(BSDC_INFLATE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
#define INF_CLOCK(k)                           \
    if (lane == 0 && phase_acc) {              \
        const uint64_t now = wall_clock64();   \
        phase_acc[k] += now - phase_t;         \
        phase_t = now;                         \
    }
#else
#define INF_CLOCK(k) (void)0
#endif

// One BGZF block by nl lanes sharing W (the kernel: a wave and LDS; the host twin: lane 0 of 1).
// Returns the block's status on every lane; the window W.out + shift (shift < 16) holds its bytes.
HD int run_block(Work &W, const uint8_t *comp, const bsdc_inflate_block &b, int shift, int lane, int nl,
                 uint64_t *phase_acc) {
    const int32_t n = b.clen, isize = b.isize;
    const uint8_t *cb = comp + b.src;
    uint8_t *win = W.out + shift;
#if defined(BSDC_INFLATE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
    uint64_t phase_t = wall_clock64();
#endif
    if (lane == 0) {
        W.st.bitpos = W.st.outpos = W.st.nt = W.st.err = 0;
        W.st.phase = PH_HEADER;
        W.st.bfinal = 0;
    }
    INF_SYNC();
    for (;;) {
        if (W.st.err || W.st.phase == PH_DONE) break;  // (uniform: read after a barrier)
        const uint8_t *bw = cb;
        int32_t base = 0, wlen = n;
#ifdef __HIP_DEVICE_COMPILE__
        {
            // the window starts at the dword of `comp` that holds the next bit; whole dwords inside the
            // block as dword loads, the ends by bytes; nothing outside [src, src + clen) is read
            const int32_t at = W.st.bitpos >> 3;
            base = at - (int32_t)(((uintptr_t)cb + (uintptr_t)at) & 3);
            wlen = kCompWin;
            for (int w = lane; w < kCompWin / 4; w += nl) {
                const int32_t o = base + 4 * w;
                uint32_t v = 0;
                if (o >= 0 && o + 4 <= n) {
                    v = *reinterpret_cast<const uint32_t *>(cb + o);
                } else {
                    for (int k = 0; k < 4; k++)
                        if (o + k >= 0 && o + k < n) v |= (uint32_t)cb[o + k] << (8 * k);
                }
                reinterpret_cast<uint32_t *>(W.cw)[w] = v;
            }
            bw = W.cw;
        }
        INF_SYNC();
#endif
        if (W.st.phase == PH_HEADER) {
            if (lane == 0) {
                Bits br;
                br.start(bw, base, wlen, n, W.st.bitpos);
                step_header(br, W.st, W.T);
                if (!W.st.err && W.st.kind == KIND_STORED) W.st.err = stored_check(W.st, n, isize);
            }
            INF_SYNC();
            if (W.st.err) break;
            if (W.st.kind == KIND_STORED) {
                const int32_t from = W.st.stored_from, len = W.st.stored_len, p = W.st.outpos;
                for (int i = lane; i < len; i += nl) win[p + i] = cb[from + i];
                INF_SYNC();
                if (lane == 0) {
                    W.st.outpos = p + len;
                    W.st.bitpos = (from + len) * 8;
                    W.st.phase = W.st.bfinal ? PH_DONE : PH_HEADER;
                }
            } else {
                huff_build(W.T.lens, W.st.hlit, W.T.lit, lane, nl, &W.st.err);
                huff_build(W.T.lens + W.st.hlit, W.st.hdist, W.T.dist, lane, nl, &W.st.err);
                if (lane == 0) W.st.phase = PH_TOKENS;
            }
            INF_SYNC();
            INF_CLOCK(0);
        } else {
            if (lane == 0) {
                Bits br;
                br.start(bw, base, wlen, n, W.st.bitpos);
                step_tokens(br, W.st, W.T, W.tok, W.tpos, isize);
            }
            INF_SYNC();
            INF_CLOCK(1);
            if (W.st.err) break;
            const int nt = W.st.nt;
            for (int k = lane; k < nt; k += nl)
                if (!(W.tok[k] >> 31)) win[W.tpos[k]] = (uint8_t)W.tok[k];
            INF_SYNC();
            for (int k = 0; k < nt; k++) {  // (uniform: every lane reads the same token)
                const uint32_t x = W.tok[k];
                if (!(x >> 31)) continue;
                copy_match(win, W.tpos[k], (int)((x >> 16) & 0x1FF), (int)(x & 0xFFFF), lane, nl);
                INF_SYNC();
            }
            INF_CLOCK(2);
        }
    }
    INF_SYNC();
    int err = W.st.err;
    if (!err && W.st.outpos != isize) err = BSDC_INFLATE_ESHORT;
    return err;
}

}  // namespace inf

namespace {

#ifdef BSDC_INFLATE_PHASES
__device__ uint64_t g_inflate_phase[8192 * 4];
#endif

__global__ __launch_bounds__(64) void k_inflate(const uint8_t *__restrict__ comp, int64_t n_comp,
                                                const bsdc_inflate_block *__restrict__ blk, uint8_t *__restrict__ out,
                                                int64_t n_out, int32_t *__restrict__ status) {
    __shared__ inf::Work W;
    const int lane = threadIdx.x;
    const bsdc_inflate_block b = blk[blockIdx.x];
    if (!inf::block_in_range(b, n_comp, n_out)) {
        if (lane == 0) status[blockIdx.x] = BSDC_INFLATE_ERANGE;
        return;
    }
    uint64_t *acc = nullptr;
#ifdef BSDC_INFLATE_PHASES
    if (blockIdx.x < 8192) {
        acc = g_inflate_phase + blockIdx.x * 4;
        if (lane == 0) acc[0] = acc[1] = acc[2] = acc[3] = 0;
    }
#endif
    // the window sits at the destination's misalignment, so LDS and `out` agree mod 16 in round W
    uint8_t *dst = out + b.dst;
    const int a = (int)((uintptr_t)dst & 15);
    const int err = inf::run_block(W, comp, b, a, lane, 64, acc);
    if (!err) {
        const uint8_t *w = W.out + a;
        const int n = b.isize;
        const int head = ::min(n, (16 - a) & 15);
        if (lane < head) dst[lane] = w[lane];
        const int body = (n - head) >> 4;
        for (int i = lane; i < body; i += 64)
            *reinterpret_cast<uint4 *>(dst + head + 16 * i) = *reinterpret_cast<const uint4 *>(w + head + 16 * i);
        const int done = head + 16 * body;
        if (done + lane < n) dst[done + lane] = w[done + lane];  // (a tail of < 16 bytes)
#ifdef BSDC_INFLATE_PHASES
        if (lane == 0 && acc) acc[3] = wall_clock64();  // (the write-out's start; the host takes the kernel's end)
#endif
    }
    if (lane == 0) status[blockIdx.x] = err;
}

}  // namespace

extern "C" {

// include/bsdc.h: the blocks' bytes on the device, one workgroup per block.
int32_t bsdc_bgzf_inflate(const uint8_t *comp, int64_t n_comp, const bsdc_inflate_block *blk, int64_t nblk, uint8_t *out,
                          int64_t n_out, int32_t *status, void *stream) {
    if (nblk == 0) return 0;
    if (nblk < 0 || nblk > 0x7FFFFFFF || n_comp < 0 || n_out < 0 || !blk || !status || (!comp && n_comp) || (!out && n_out))
        return BSDC_EINVAL;
    hipLaunchKernelGGL(k_inflate, dim3((unsigned)nblk), dim3(64), 0, (hipStream_t)stream, comp, n_comp, blk, out, n_out,
                       status);
    return hipGetLastError() == hipSuccess ? 0 : BSDC_EDEVICE;
}

// The same blocks through the same functions on the host, one after the other (host pointers).
int32_t bsdc_bgzf_inflate_host(const uint8_t *comp, int64_t n_comp, const bsdc_inflate_block *blk, int64_t nblk,
                               uint8_t *out, int64_t n_out, int32_t *status) {
    if (nblk == 0) return 0;
    if (nblk < 0 || n_comp < 0 || n_out < 0 || !blk || !status || (!comp && n_comp) || (!out && n_out)) return BSDC_EINVAL;
    std::vector<inf::Work> work(1);
    inf::Work &W = work[0];
    for (int64_t i = 0; i < nblk; i++) {
        const bsdc_inflate_block b = blk[i];
        if (!inf::block_in_range(b, n_comp, n_out)) {
            status[i] = BSDC_INFLATE_ERANGE;
            continue;
        }
        const int err = inf::run_block(W, comp, b, 0, 0, 1, nullptr);
        if (!err && b.isize) memcpy(out + b.dst, W.out, (size_t)b.isize);
        status[i] = err;
    }
    return 0;
}

#ifdef BSDC_INFLATE_PHASES
int32_t bsdc_inflate_phases(uint64_t *host, int64_t n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_inflate_phase), (size_t)n * sizeof(uint64_t)) == hipSuccess ? 0 : -5;
}
#endif

}  // extern "C"
