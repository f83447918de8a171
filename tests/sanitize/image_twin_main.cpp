// The family-image gather's host twin (bsdc_image_gather_host, csrc/bsdc_image.hip) as a stand-alone
// program for the sanitizers: raw, the table and both images in heap buffers of their exact sizes,
// so that any read or write past them is caught.  Host code only; built without hipcc the included
// file holds the twin alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       tests/sanitize/image_twin_main.cpp -o image_twin && ./image_twin
// Cases: l_seq 0..40 and 149..152 (odd and even: QUAL's offset), every skip 0..3, kept lengths 0,
// 1, 2, 7, 8, 9, 15, 16, 17 and the whole rest, SEQ at every src % 4 (the first record at raw's
// first byte, the last one ending at its last), quality bytes 0, 93, 127, 128, 255, slots back to
// back from 32 (neighbours share dwords of the packed image; the first slot past 0) with the last
// record ending at the image's end; the images are compared with a base-by-base statement.  Then
// every out-of-range table entry, which must be refused with nothing written.
#include "../../bsseqconsensusreads_amd/csrc/bsdc_image.hip"

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
        std::printf("FAIL %s (%ld): %s\n", what, i, bsdc_image_last_error());
    }
}

struct Heap {  // exact-size heap buffers (malloc: 16-byte aligned)
    uint8_t *raw, *seq, *qual;
    bsdc_image_rec *recs;
    int64_t n_raw, n_rec, n_slots;
    Heap(const std::vector<uint8_t> &r, const std::vector<bsdc_image_rec> &t, int64_t ns)
        : n_raw((int64_t)r.size()), n_rec((int64_t)t.size()), n_slots(ns) {
        raw = (uint8_t *)std::malloc(r.size() ? r.size() : 1);
        recs = (bsdc_image_rec *)std::malloc(t.size() * sizeof(bsdc_image_rec) + 1);
        seq = (uint8_t *)std::malloc((size_t)(ns / 2) + (ns ? 0 : 1));
        qual = (uint8_t *)std::malloc((size_t)ns + (ns ? 0 : 1));
        if (!r.empty()) memcpy(raw, r.data(), r.size());
        if (!t.empty()) memcpy(recs, t.data(), t.size() * sizeof(bsdc_image_rec));
        memset(seq, 0xA5, (size_t)(ns / 2));
        memset(qual, 0xA5, (size_t)ns);
    }
    ~Heap() {
        std::free(raw);
        std::free(recs);
        std::free(seq);
        std::free(qual);
    }
    int32_t run() { return bsdc_image_gather_host(nullptr, raw, n_raw, recs, n_rec, n_slots, seq, qual); }
};

}  // namespace

int main() {
    static const uint8_t qedge[5] = {0, 93, 127, 128, 255};
    static const int keep[9] = {0, 1, 2, 7, 8, 9, 15, 16, 17};
    std::vector<uint8_t> raw;
    std::vector<bsdc_image_rec> tab;
    std::vector<int> lens;
    for (int l = 0; l <= 40; l++) lens.push_back(l);
    for (int rep = 0; rep < 4; rep++)
        for (int l = 149; l <= 152; l++) lens.push_back(l);
    int64_t slot = 32;
    for (size_t i = 0; i < lens.size(); i++) {
        const int l = lens[i];
        if (i) {  // any alignment of SEQ; the first record starts raw, the last one ends it
            const int pad = (int)(rnd() % 4);
            for (int k = 0; k < pad; k++) raw.push_back((uint8_t)rnd());
        }
        bsdc_image_rec r;
        r.src = (int64_t)raw.size();
        r.l_seq = l;
        r.skip = l ? (int32_t)(i % 4 > (size_t)l ? 0 : i % 4) : 0;
        if (r.skip > l) r.skip = l;
        const int rest = l - r.skip;
        int len = keep[i % 9];
        if (len > rest || i % 3 == 0) len = rest;
        r.len = len;
        r.slot = (uint32_t)slot;
        slot += (len + 2 + 3) / 4 * 4;
        if (i % 6 == 5) slot = (slot + 31) / 32 * 32;  // a family's alignment
        for (int k = 0; k < (l + 1) / 2; k++) raw.push_back((uint8_t)rnd());
        for (int k = 0; k < l; k++) raw.push_back(i % 2 ? qedge[rnd() % 5] : (uint8_t)rnd());
        tab.push_back(r);
    }
    // the image ends with the last record's last base's dword: n_slots the least multiple of 8
    const bsdc_image_rec &last = tab.back();
    const int64_t n_slots = ((int64_t)last.slot + 1 + last.len + 7) / 8 * 8;
    {
        Heap h(raw, tab, n_slots);
        expect(h.run() == 0, "the cases");
        std::vector<uint8_t> code((size_t)n_slots, 0), q((size_t)n_slots, 0);
        for (const bsdc_image_rec &r : tab)
            for (int j = 0; j < r.len; j++) {
                const uint8_t b = raw[(size_t)(r.src + (r.skip + j) / 2)];
                code[(size_t)(r.slot + 1 + j)] = ((r.skip + j) & 1) ? (b & 15) : (b >> 4);
                q[(size_t)(r.slot + 1 + j)] = raw[(size_t)(r.src + (r.l_seq + 1) / 2 + r.skip + j)];
            }
        for (int64_t s = 0; s < n_slots; s++) expect(h.qual[s] == q[(size_t)s], "qual image", (long)s);
        for (int64_t s = 0; s < n_slots / 2; s++)
            expect(h.seq[s] == (uint8_t)(code[(size_t)(2 * s)] << 4 | code[(size_t)(2 * s + 1)]), "seq image", (long)s);
    }
    {  // an empty table and empty images
        Heap h(raw, std::vector<bsdc_image_rec>(), 0);
        expect(h.run() == 0, "empty table");
    }
    // every out-of-range entry is refused before anything is written
    struct Bad {
        const char *what;
        size_t i;
        int field;  // 0 src, 1 l_seq, 2 skip, 3 len, 4 slot
        int64_t v;
    };
    const int64_t n_raw = (int64_t)raw.size();
    const size_t big = tab.size() - 1;
    const Bad bad[] = {
        {"src", 3, 0, -1}, {"src", big, 0, n_raw - 1}, {"src", 5, 0, n_raw + 1}, {"src", 9, 0, INT64_MAX},
        {"src", 9, 0, INT64_MIN}, {"src", 5, 1, -1}, {"src", 5, 1, INT32_MAX}, {"src", big, 1, tab[big].l_seq + 1},
        {"skip + len", 7, 2, -1}, {"skip + len", 7, 3, -1}, {"skip + len", 8, 3, tab[8].l_seq - tab[8].skip + 1},
        {"skip + len", 8, 2, INT32_MAX}, {"skip + len", 8, 3, INT32_MAX}, {"skip + len", 8, 2, INT32_MIN},
        {"multiple of 4", 2, 4, tab[2].slot + 1}, {"multiple of 4", 2, 4, tab[2].slot + 2}, {"multiple of 4", 2, 4, tab[2].slot + 3},
        {"slot + 1 + len", big, 4, tab[big].slot + 8}, {"slot + 1 + len", big, 4, 0xFFFFFFFCll}, {"slot + 1 + len", 12, 4, n_slots},
    };
    for (const Bad &b : bad) {
        std::vector<bsdc_image_rec> t = tab;
        bsdc_image_rec &r = t[b.i];
        if (b.field == 0) r.src = b.v;
        if (b.field == 1) r.l_seq = (int32_t)b.v;
        if (b.field == 2) r.skip = (int32_t)b.v;
        if (b.field == 3) r.len = (int32_t)b.v;
        if (b.field == 4) r.slot = (uint32_t)b.v;
        Heap h(raw, t, n_slots);
        expect(h.run() == BSDC_EINVAL, b.what, (long)b.i);
        expect(std::string(bsdc_image_last_error()).find(b.what) != std::string::npos, "message names the field", (long)b.i);
        bool clean = true;
        for (int64_t s = 0; s < n_slots; s++) clean &= h.qual[s] == 0xA5 && h.seq[s / 2] == 0xA5;
        expect(clean, "nothing written on a refusal", (long)b.i);
    }
    {
        Heap h(raw, tab, n_slots + 4);  // (n_slots not a multiple of 8)
        expect(h.run() == BSDC_EINVAL, "n_slots % 8");
    }
    if (fails) return 1;
    std::printf("image twin ok: %zu records, %lld raw bytes, %lld slots, %zu refusals\n", tab.size(), (long long)n_raw,
                (long long)n_slots, sizeof(bad) / sizeof(bad[0]));
    return 0;
}
