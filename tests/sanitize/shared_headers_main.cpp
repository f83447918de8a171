// The two shared headers (csrc/bsdc_ssrows.h, csrc/bsdc_devtext.h) as a stand-alone program for the
// sanitizers: the one statement of the consensus-row views and per-read values, and the dword
// helpers and record writer of the output passes, on heap buffers of their exact sizes.  Host code
// only: built without hipcc the headers hold their plain C++ halves.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/sanitize/shared_headers_main.cpp -o shared_headers && ./shared_headers
// Cases: the duplex column rule (equal calls, a / b the higher quality, different calls at equal
// quality, an N against a base, bits above the nibble); the end selection (molecular, duplex with
// both rows, AB only, BA only, both ends) and the row addresses with and without a wide row, read
// at the buffers' last elements; the rate (1 / 3, 0 / 0, 5 / 0) from every sum type; load4 and
// can4 at every byte of a buffer and one byte either side; store_record for records of 1, 4, 5 and
// 9 bytes at the four start offsets, `cap` at every byte, one lane and 64.
#include "../../bsseqconsensusreads_amd/csrc/bsdc_devtext.h"
#include "../../bsseqconsensusreads_amd/csrc/bsdc_ssrows.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

using namespace bsdc_devtext;
using namespace bsdc_ssrows;

int fails = 0;
void expect(bool ok, const char *what, long i = -1, long j = -1) {
    if (!ok) {
        fails++;
        std::printf("FAIL %s (%ld, %ld)\n", what, i, j);
    }
}

template <class T>
T *heap(size_t n) {  // exactly n elements (malloc: 16-byte aligned), bytes 1, 2, 3, ..
    T *p = (T *)std::malloc(n * sizeof(T));
    for (size_t i = 0; i < n * sizeof(T); i++) ((uint8_t *)p)[i] = (uint8_t)(i * 37 + 1);
    return p;
}

uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

void column_rule() {
    // a: depth 5, 1 error; b: depth 3, 2 errors
    struct {
        uint32_t ab, aq, bb, bq, e;
        const char *what;
    } const cases[] = {
        {1, 30, 1, 20, 1 + 2, "equal calls: both strands' errors"},
        {1, 30, 2, 20, 1 + 3, "a higher quality: b disagrees, all of its reads"},
        {1, 20, 2, 30, 5 + 2, "b higher quality: a disagrees, all of its reads"},
        {1, 25, 2, 25, 1 + 3, "equal quality: a's call is the raw one"},
        {15, 2, 4, 30, 5 + 2, "an N against a base: the base of the higher quality"},
        {4, 30, 15, 2, 1 + 3, "a base against an N"},
        {0x31, 30, 0xF1, 20, 1 + 2, "bits above the nibble do not count"},
    };
    for (const auto &c : cases) {
        const Col r = duplex_col(c.ab, c.aq, 5, 1, c.bb, c.bq, 3, 2);
        expect(r.d == 8 && r.e == c.e, c.what, (long)r.d, (long)r.e);
    }
}

void end_selection() {
    const int F = 3, stride = 16, W = 2;
    struct {
        uint8_t *ss_base, *ss_qual, *ss_depth, *ss_err;
        uint16_t *ss_wdepth, *ss_werr;
        int32_t stride;
    } A{heap<uint8_t>(4 * F * stride), heap<uint8_t>(4 * F * stride), heap<uint8_t>(4 * F * stride),
        heap<uint8_t>(4 * F * stride), heap<uint16_t>(4 * W * stride), heap<uint16_t>(4 * W * stride), stride};
    uint16_t *ss_len = heap<uint16_t>(4 * F);
    const int64_t f = F - 1;  // the last family: its rows end at the buffers' ends
    for (int e = 0; e < 2; e++) {
        const End m = end_rows(1, nullptr, f, e);  // molecular: ss_len is not read
        expect(m.a == e && !m.two, "molecular: row e, no b", e);
        for (int have = 0; have < 4; have++) {  // bit 0: the AB row has a read, bit 1: the BA row
            for (int s = 0; s < 4; s++) ss_len[4 * f + s] = 0;
            ss_len[4 * f + e] = (have & 1) ? 7 : 0;
            ss_len[4 * f + 3 - e] = (have & 2) ? 9 : 0;
            const End d = end_rows(0, ss_len, f, e);
            expect(d.b == 3 - e, "duplex: b is row 3 - e", e, have);
            expect(d.two == (have == 3), "duplex: two = both present", e, have);
            // (neither present: row 3 - e as well, as empty as row e)
            expect(d.a == ((have & 1) ? e : 3 - e), "duplex: a = the AB row, or row 3 - e when AB is empty", e, have);
        }
    }
    for (int s = 0; s < 4; s++) {
        const size_t at = (size_t)(4 * f + s) * stride;
        const Row r = row_of(A, f, s, -1);
        expect(r.b == A.ss_base + at && r.q == A.ss_qual + at && r.d8 == A.ss_depth + at && r.e8 == A.ss_err + at,
               "row (f, s) at (4 f + s) * stride", s);
        expect(!r.d16 && !r.e16, "no wide row", s);
        expect(r.d(stride - 1) == A.ss_depth[at + stride - 1] && r.e(stride - 1) == A.ss_err[at + stride - 1],
               "d / e from the bytes", s);
        for (int w = 0; w < W; w++) {
            const size_t aw = (size_t)(4 * w + s) * stride;
            const Row x = row_of(A, f, s, w);
            expect(x.b == r.b && x.q == r.q && x.d8 == r.d8 && x.e8 == r.e8, "a wide row leaves the byte rows", s, w);
            expect(x.d16 == A.ss_wdepth + aw && x.e16 == A.ss_werr + aw, "wide row at (4 w + s) * stride", s, w);
            expect(x.d(stride - 1) == A.ss_wdepth[aw + stride - 1] && x.e(stride - 1) == A.ss_werr[aw + stride - 1],
                   "d / e from the wide row", s, w);
            expect(x.d(0) > 255u, "a wide value past a byte", s, w);
        }
    }
    std::free(A.ss_base), std::free(A.ss_qual), std::free(A.ss_depth), std::free(A.ss_err);
    std::free(A.ss_wdepth), std::free(A.ss_werr), std::free(ss_len);
}

template <class T>
void rate_of(const char *type) {
    expect(bits(read_rate((T)1, (T)3)) == 0x3EAAAAABu, type, 1, 3);
    const float n = read_rate((T)0, (T)0);
    expect(n != n, type, 0, 0);
    expect(bits(read_rate((T)5, (T)0)) == 0x7F800000u, type, 5, 0);
}

void dword_loads() {
    const int n = 16;
    // the buffer alone in its heap block: a read past either end is the sanitizer's
    uint8_t *buf = heap<uint8_t>(n);
    for (int a = 0; a + 4 <= n; a++) {
        uint32_t want;
        memcpy(&want, buf + a, 4);  // (little-endian host)
        expect(can4(buf, n, buf + a), "can4 inside the buffer", a);
        expect(load4(buf + a) == want, "load4", a);
    }
    expect(can4(buf, n, buf + n - 4), "can4 at the last four bytes");
    for (int a = n - 3; a <= n; a++) expect(!can4(buf, n, buf + a), "can4 past the last four bytes", a);
    expect(!can4(buf, 15, buf + 9) && can4(buf, 15, buf + 8), "can4: the second aligned dword must be whole", 15);
    std::free(buf);
    // one byte before: the buffer inside a larger block, so that the pointer itself is a valid one
    uint8_t *block = heap<uint8_t>(n + 4);
    expect(!can4(block + 4, n, block + 3) && can4(block + 4, n, block + 4), "can4 one byte before the buffer");
    std::free(block);
}

void record_stores() {
    const int sizes[] = {1, 4, 5, 9};
    const int lanes[] = {1, 64};
    const int lead = 8, guard = 4;
    for (int size : sizes)
        for (int ho = 0; ho < 4; ho++)
            for (int nl : lanes) {
                const int64_t o = lead + ho;
                const int len = (int)o + size + guard;
                for (int64_t cap = 0; cap <= o + size + guard; cap++) {
                    uint8_t *dst = (uint8_t *)std::malloc((size_t)len);  // (16-byte aligned: the start's offset is ho)
                    memset(dst, 0xEE, (size_t)len);
                    int calls = 0;
                    auto dword_of = [&](int i0) {  // the record's bytes 3 i + 1; 0xAA outside it
                        calls++;
                        uint32_t v = 0;
                        for (int b = 0; b < 4; b++) {
                            const int i = i0 + b;
                            v |= (uint32_t)(i >= 0 && i < size ? (uint8_t)(3 * i + 1) : 0xAAu) << (8 * b);
                        }
                        return v;
                    };
                    for (int lane = 0; lane < nl; lane++) store_record(dst, o, size, cap, lane, nl, dword_of);
                    expect(calls == (ho + size + 3) / 4, "one dword_of per destination dword", size, ho);
                    for (int p = 0; p < len; p++) {
                        const bool in = p >= o && p < o + size && p < cap;
                        const uint8_t want = in ? (uint8_t)(3 * (p - o) + 1) : 0xEE;
                        if (dst[p] != want) {
                            expect(false, in ? "a record byte" : "a byte outside the record or at or past cap", size * 10 + ho,
                                   cap * 100 + p);
                            break;
                        }
                    }
                    std::free(dst);
                }
            }
}

}  // namespace

int main() {
    column_rule();
    end_selection();
    rate_of<uint32_t>("rate of u32 sums");
    rate_of<uint64_t>("rate of u64 sums");
    rate_of<int64_t>("rate of i64 sums");
    dword_loads();
    record_stores();
    expect(add33x4(0x5d00ff7fu) == 0x7e2120a0u, "add33x4: no carry between bytes");
    expect(nt16x4(0x0f080201u) == 0x4e544341u, "nt16x4");  // A C T N
    if (fails) return 1;
    std::printf("shared headers ok\n");
    return 0;
}
