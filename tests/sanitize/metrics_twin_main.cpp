// The metrics reduction's host twin (bsdc_metrics_host, csrc/bsdc_metrics.hip) as a stand-alone
// program for the sanitizers: every input row and the accumulator in heap buffers of their exact
// sizes, so that any read or write past them is caught.  Host code only; built without hipcc the
// included file holds the twin alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       tests/sanitize/metrics_twin_main.cpp -o metrics_twin && ./metrics_twin
// Cases: strides 16, 32 and 528 with cycles 512 and 2, duplex and molecular; lengths 0, 1, 15, 16,
// 17, the stride itself (the last family's rows end at the buffers' ends) and, at stride 528, 511
// to 513; one-strand and no-strand ends; a wide row for every third family, the last one the
// table's last row; families that are not emitted; and the bad families -- a length of stride + 1
// and of 65535, a wide row at n_wide and at 2^30 -- which must be counted as skipped and never read
// (their rows, were they read, lie past the buffers).  The totals are checked against the
// invariants of DESIGN.md 3.9; then the refusals.
#include "../../bsseqconsensusreads_amd/csrc/bsdc_metrics.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 24);
}

int fails = 0;
void expect(bool ok, const char *what, long i = -1) {
    if (!ok) {
        fails++;
        std::printf("FAIL %s (%ld): %s\n", what, i, bsdc_metrics_last_error());
    }
}

template <class T>
T *heap(size_t n) {  // exactly n elements (malloc: 16-byte aligned), random bytes
    T *p = (T *)std::malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n * sizeof(T); i++) ((uint8_t *)p)[i] = (uint8_t)rnd();
    return p;
}

void run_case(int stride, int cycles, int kind, int F) {
    const int lens[] = {0, 1, 15, 16, 17, stride, 511, 512, 513};
    int W = 0;
    std::vector<int32_t> wide(F, -1);
    for (int f = 0; f < F; f++)
        if (f % 3 == 2) wide[f] = W++;
    bsdc_consensus o;
    memset(&o, 0, sizeof o);
    o.stride = stride;
    o.status = heap<uint8_t>(F);
    o.len = heap<uint16_t>(2 * F);
    o.seq = heap<uint8_t>((size_t)F * stride);
    o.qual = heap<uint8_t>((size_t)2 * F * stride);
    o.ss_len = heap<uint16_t>(4 * F);
    o.ss_base = heap<uint8_t>((size_t)4 * F * stride);
    o.ss_qual = heap<uint8_t>((size_t)4 * F * stride);
    o.ss_depth = heap<uint8_t>((size_t)4 * F * stride);
    o.ss_err = heap<uint8_t>((size_t)4 * F * stride);
    int32_t *wd = heap<int32_t>(F);
    o.ss_wdepth = heap<uint16_t>((size_t)4 * W * stride);
    o.ss_werr = heap<uint16_t>((size_t)4 * W * stride);
    for (size_t i = 0; i < (size_t)4 * W * stride; i++) o.ss_wdepth[i] &= 32767, o.ss_werr[i] &= 32767;
    uint64_t want_rec = 0, want_len[2] = {0, 0}, want_skip = 0, want_em = 0;
    for (int f = 0; f < F; f++) {
        wd[f] = wide[f];
        o.status[f] = (uint8_t)((rnd() & 0xFE) | (f % 5 != 3));
        bool bad = false;
        for (int e = 0; e < 2; e++) {
            int L = lens[rnd() % 9];
            if (L > stride) L = stride;
            if (f == F - 1) L = stride;
            o.len[2 * f + e] = (uint16_t)L;
        }
        if (f % 11 == 4) o.len[2 * f + (f & 1)] = (uint16_t)(f % 2 ? stride + 1 : 65535), bad = true;
        if (f % 11 == 8 && wide[f] >= 0) wd[f] = f % 2 ? W : (1 << 30), bad = true;
        for (int s = 0; s < 4; s++) o.ss_len[4 * f + s] = (uint16_t)(rnd() % 3 ? 1 + rnd() % stride : 0);
        if (!(o.status[f] & 1)) continue;
        want_em++;
        if (bad) {
            want_skip++;
            continue;
        }
        want_rec += 2;
        want_len[0] += o.len[2 * f], want_len[1] += o.len[2 * f + 1];
    }
    o.ss_wide = wd;
    const int64_t n = bsdc_metrics_words(cycles);
    uint64_t *acc = heap<uint64_t>((size_t)n);
    memset(acc, 0, (size_t)n * 8);
    expect(bsdc_metrics_host(nullptr, &o, F, W, kind, cycles, acc) == 0, "twin", stride);
    expect(acc[BSDC_METRICS_FAMILIES] == (uint64_t)F && acc[BSDC_METRICS_EMITTED] == want_em, "families", stride);
    expect(acc[BSDC_METRICS_RECORDS] == want_rec && acc[BSDC_METRICS_SKIPPED] == want_skip, "records / skipped", stride);
    for (int e = 0; e < 2; e++) {
        for (int k = 0; k < 3; k++) {
            uint64_t d = 0, r = 0;
            for (int i = 0; i < 256; i++) d += acc[BSDC_METRICS_DEPTH_HIST + (k * 2 + e) * 256 + i];
            for (int i = 0; i < 102; i++) r += acc[BSDC_METRICS_RATE_HIST + (k * 2 + e) * 102 + i];
            expect(d == want_rec / 2 && r == want_rec / 2, "one count per record", k);
        }
        uint64_t q = 0, c = 0;
        for (int i = 0; i < 95; i++) q += acc[BSDC_METRICS_QUAL_HIST + e * 95 + i];
        for (int i = 0; i < cycles; i++) {
            const uint64_t *row = acc + BSDC_METRICS_BY_CYCLE + ((size_t)e * cycles + i) * 6;
            c += row[0];
            expect(row[1] <= row[0] && row[5] <= row[0], "no-calls and disagreements within the covered", i);
        }
        expect(q == want_len[e] && c == want_len[e], "columns", e);
    }
    // a second call adds the same again
    std::vector<uint64_t> once(acc, acc + n);
    expect(bsdc_metrics_host(nullptr, &o, F, W, kind, cycles, acc) == 0, "twin again", stride);
    for (int64_t i = 0; i < n; i++)
        if (acc[i] != 2 * once[i]) {
            expect(false, "two calls add up", (long)i);
            break;
        }
    // the filter's counters
    uint8_t *filt = heap<uint8_t>(F);
    uint16_t *masked = heap<uint16_t>(2 * F);
    expect(bsdc_metrics_filter_host(nullptr, o.status, filt, masked, F, acc) == 0, "filter twin", stride);
    std::free(filt), std::free(masked), std::free(acc);
    std::free(o.status), std::free(o.len), std::free(o.seq), std::free(o.qual), std::free(o.ss_len), std::free(o.ss_base);
    std::free(o.ss_qual), std::free(o.ss_depth), std::free(o.ss_err), std::free(wd), std::free(o.ss_wdepth), std::free(o.ss_werr);
}

void refusals() {
    bsdc_consensus o;
    memset(&o, 0, sizeof o);
    uint64_t *acc = heap<uint64_t>((size_t)bsdc_metrics_words(512));
    uint8_t *buf = heap<uint8_t>(64);
    o.stride = 16;
    o.status = o.seq = o.qual = o.ss_base = o.ss_qual = o.ss_depth = o.ss_err = buf;
    o.len = o.ss_len = (uint16_t *)buf;
    expect(bsdc_metrics_host(nullptr, &o, 0, 0, 0, 512, acc) == 0, "empty batch");
    expect(bsdc_metrics_host(nullptr, &o, 0, 0, 0, 1, acc) == BSDC_EINVAL, "cycles 1");
    expect(bsdc_metrics_host(nullptr, &o, 0, 0, 0, 512, nullptr) == BSDC_EINVAL, "null acc");
    expect(bsdc_metrics_host(nullptr, nullptr, 0, 0, 0, 512, acc) == BSDC_EINVAL, "null out");
    o.stride = 24;
    expect(bsdc_metrics_host(nullptr, &o, 0, 0, 0, 512, acc) == BSDC_EINVAL, "stride 24");
    o.stride = 16, o.ss_depth = nullptr;
    expect(bsdc_metrics_host(nullptr, &o, 0, 0, 0, 512, acc) == BSDC_EINVAL, "null ss_depth");
    expect(bsdc_metrics_words(1) == BSDC_EINVAL && bsdc_metrics_words(2) == BSDC_METRICS_BY_CYCLE + 24, "words");
    std::free(acc), std::free(buf);
}

}  // namespace

int main() {
    for (int kind = 0; kind < 2; kind++) {
        run_case(16, 512, kind, 40);
        run_case(32, 2, kind, 67);
        run_case(528, 512, kind, 45);
        run_case(528, 2, kind, 23);
    }
    refusals();
    if (fails) return 1;
    std::printf("metrics twin ok\n");
    return 0;
}
