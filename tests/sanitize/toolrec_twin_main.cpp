// The tool-stage record writer's host twin (bsdc_toolrec_host, csrc/bsdc_toolrec.hip) as a
// stand-alone program for the sanitizers: the dump, the table, the names, the ops, the aux bytes and
// the destination in heap buffers of their exact sizes, so that any read or write past them is
// caught.  Host code only; built without hipcc the included file holds the twin alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       tests/sanitize/toolrec_twin_main.cpp -o toolrec_twin && ./toolrec_twin
// Cases, the shapes of tests/toolrec_inputs.py: 0, 1, 63, 64 and 65 records; lengths 1, 2, 15, 16,
// 17, 255, 256, 257 and 65529; names of 1..8 and 254 bytes; aux of 0..3 and 70,000 bytes, its
// buffer no multiple of 4 long; every tag value 0..15; 0 to 3 ops with a last op of length 1 and
// more; the last record's dump slot ending at the dump's end; a destination of exactly the bound.
// Every record's block_size is checked against its offsets, and the bytes past the total stay.
// Then a dump slot that leaves the dump (refused, nothing written), and the refusals.
// long_cigars: 64, 65, 129 and 65,533 ops (more than the kernel's wavefront has lanes, up to the most
// a record holds) and reference lengths past 2^32.  shared_entries: table entries on the same bytes,
// so that the records outgrow a destination of exactly the bound, which is the heap block's size.
#include "../../bsseqconsensusreads_amd/csrc/bsdc_toolrec.hip"

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
        std::printf("FAIL %s (%ld): %s\n", what, i, bsdc_toolrec_last_error());
    }
}

template <class T>
T *heap(size_t n) {  // exactly n elements (malloc: 16-byte aligned), random bytes
    T *p = (T *)std::malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n * sizeof(T); i++) ((uint8_t *)p)[i] = (uint8_t)rnd();
    return p;
}

void run_case(int n, bool big, bool break_last) {
    const int lens[] = {1, 2, 15, 16, 17, 255, 256, 257, 65529};
    const int nls[] = {1, 2, 3, 4, 5, 6, 7, 8, 254};
    std::vector<bsdc_toolrec_rec> tab(n ? n : 1);  // (never a null table)
    std::vector<int> L(n);
    std::vector<uint32_t> rec(4 * (size_t)(n ? n : 1));
    int64_t nb = 0, no = 0, ab = 0, nd = 0;
    for (int r = 0; r < n; r++) {
        bsdc_toolrec_rec &e = tab[r];
        memset(&e, 0, sizeof e);
        L[r] = lens[big && r == n / 2 ? 8 : rnd() % 8];
        e.name_len = (uint8_t)nls[rnd() % 9], e.name_off = nb, nb += e.name_len;
        e.n_cig = (int32_t)(rnd() % 4), e.cig_off = no, no += e.n_cig;
        e.aux_len = big && r == n / 2 ? 70000 : (int32_t)(rnd() % 4) + (rnd() % 3 ? 40 : 0), e.aux_off = ab, ab += e.aux_len;
        e.ref_id = (int32_t)(rnd() % 3), e.next_ref_id = -1, e.next_pos = (int32_t)rnd(), e.tlen = -(int32_t)(rnd() % 1000);
        e.flag = (uint16_t)rnd(), e.mapq = (uint8_t)rnd();
        rec[4 * r] = (uint32_t)nd;
        nd += r == n - 1 ? (L[r] + 3) / 4 * 4 : (L[r] + 2 + 3) / 4 * 4;  // (the last slot ends with the dump)
    }
    bsdc_consensus o;
    memset(&o, 0, sizeof o);
    o.dump_pos = heap<int32_t>(n);
    o.dump_len = heap<uint16_t>(n);
    o.dump_tags = heap<uint8_t>(n);
    o.dump_seq = heap<uint8_t>((size_t)nd);
    o.dump_qual = heap<uint8_t>((size_t)nd);
    uint8_t *names = heap<uint8_t>((size_t)nb), *aux = heap<uint8_t>((size_t)ab);
    uint32_t *cig = heap<uint32_t>((size_t)no);
    for (int r = 0; r < n; r++) {
        o.dump_len[r] = (uint16_t)L[r], o.dump_tags[r] = (uint8_t)(r % 16), o.dump_pos[r] = (int32_t)(rnd() % (1u << 29)) - 1;
        if (tab[r].n_cig) cig[tab[r].cig_off + tab[r].n_cig - 1] = ((r & 1 ? 1u : 1 + rnd() % 300) << 4) | (rnd() % 9);
    }
    if (break_last && n) rec[4 * (n - 1)] = (uint32_t)nd - 1;  // the slot leaves the dump: l_seq 0
    const int64_t cap = bsdc_toolrec_bytes_bound(n, nb, no, ab, nd);
    const int guard = 32;
    uint8_t *dst = heap<uint8_t>((size_t)cap + guard);
    std::vector<uint8_t> before(dst, dst + cap + guard);
    int64_t *off = heap<int64_t>((size_t)n + 1);
    // (the bound is the cap; the guard behind it lies inside the heap block and must stay)
    const bool refused = break_last && n && L[n - 1] > 1;
    const int32_t rc = bsdc_toolrec_host(&o, rec.data(), n, nd, tab.data(), names, nb, cig, no, aux, ab, off, dst, cap);
    if (refused) {
        expect(rc == BSDC_EINVAL, "a dump slot that leaves the dump is refused", n);
        expect(memcmp(dst, before.data(), (size_t)cap + guard) == 0, "nothing written by a refused call", n);
        std::free(o.dump_pos), std::free(o.dump_len), std::free(o.dump_tags), std::free(o.dump_seq), std::free(o.dump_qual);
        std::free(names), std::free(aux), std::free(cig), std::free(dst), std::free(off);
        return;
    }
    expect(rc == 0, "twin", n);
    expect(off[0] == 0 && off[n] <= cap, "total within the bound", n);
    for (int r = 0; r < n; r++) {
        int32_t bs, ls;
        memcpy(&bs, dst + off[r], 4);
        memcpy(&ls, dst + off[r] + 20, 4);
        expect(off[r + 1] - off[r] == (int64_t)bs + 4, "block_size", r);
        expect(ls == L[r], "l_seq", r);
        expect(dst[off[r] + 12] == tab[r].name_len + 1, "l_read_name", r);
    }
    for (int64_t i = off[n]; i < cap + guard; i++)
        if (dst[i] != before[i]) {
            expect(false, "bytes past the total", (long)i);
            break;
        }
    std::free(o.dump_pos), std::free(o.dump_len), std::free(o.dump_tags), std::free(o.dump_seq), std::free(o.dump_qual);
    std::free(names), std::free(aux), std::free(cig), std::free(dst), std::free(off);
}

struct Batch {  // heap buffers of exact sizes for n records with one dump slot each (L bases, the last slot ends the dump)
    int n;
    std::vector<bsdc_toolrec_rec> tab;
    std::vector<uint32_t> rec;
    bsdc_consensus o;
    int64_t nd = 0;
    Batch(int n_, int L) : n(n_), tab(n_), rec(4 * (size_t)n_) {
        for (int r = 0; r < n; r++) {
            memset(&tab[r], 0, sizeof tab[r]);
            tab[r].ref_id = r % 3, tab[r].next_ref_id = -1, tab[r].flag = (uint16_t)rnd(), tab[r].mapq = (uint8_t)rnd();
            rec[4 * r] = (uint32_t)nd;
            nd += r == n - 1 ? (L + 3) / 4 * 4 : (L + 2 + 3) / 4 * 4;
        }
        memset(&o, 0, sizeof o);
        o.dump_pos = heap<int32_t>(n), o.dump_len = heap<uint16_t>(n), o.dump_tags = heap<uint8_t>(n);
        o.dump_seq = heap<uint8_t>((size_t)nd), o.dump_qual = heap<uint8_t>((size_t)nd);
        for (int r = 0; r < n; r++) o.dump_len[r] = (uint16_t)L;
    }
    ~Batch() { std::free(o.dump_pos), std::free(o.dump_len), std::free(o.dump_tags), std::free(o.dump_seq), std::free(o.dump_qual); }
};

uint32_t field32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// The `longcigar` and `hugeref` shapes of tests/toolrec_inputs.py: 64, 65, 129 and 65,533 ops under
// tags 0, 7 and 15 with a last op of length 1 and of more, then 20 and 64 ops of 268435455N (a
// reference length past 2^32: bin 0).  n_cigar_op and the bin are checked against a plain count here.
void long_cigars() {
    const int counts[] = {64, 65, 129, 65533, 20, 64};
    const int tags[] = {0, 7, 15};
    const int n = 6 * 3 * 2;
    Batch b(n, 5);
    int64_t no = 0;
    for (int r = 0; r < n; r++) {
        b.tab[r].name_len = (uint8_t)(1 + r % 4), b.tab[r].name_off = 0;
        b.tab[r].n_cig = counts[r / 6], b.tab[r].cig_off = no, no += b.tab[r].n_cig;
        b.o.dump_tags[r] = (uint8_t)tags[r / 2 % 3];
        b.o.dump_pos[r] = r / 6 >= 4 ? 1000 : (1 << 14) - 40;
    }
    uint8_t *names = heap<uint8_t>(4), *aux = heap<uint8_t>(0);
    uint32_t *cig = heap<uint32_t>((size_t)no);
    std::vector<int64_t> reflen(n);
    std::vector<int> nc(n);
    for (int r = 0; r < n; r++) {
        const bsdc_toolrec_rec &e = b.tab[r];
        const bool huge = r / 6 >= 4;
        const uint32_t t = b.o.dump_tags[r];
        int64_t s = 0;
        for (int j = 0; j < e.n_cig; j++) {
            const uint32_t kinds[] = {0, 1, 2, 3, 7, 8};
            const uint32_t k = huge ? 3 : j == e.n_cig - 1 ? 0 : kinds[rnd() % 6];
            const uint32_t len = huge ? (1u << 28) - 1 : j == e.n_cig - 1 ? (r & 1 ? 1 : 6) : 1 + rnd() % 3;
            cig[e.cig_off + j] = len << 4 | k;
            if (k != 1) s += len;
        }
        const uint32_t last = cig[e.cig_off + e.n_cig - 1] >> 4;
        const bool trim = (t & 3) == 3;
        nc[r] = e.n_cig + ((t & 6) != 0) + ((t & 8) != 0) - (trim && last <= 1);
        reflen[r] = s + ((t & 6) != 0) + ((t & 8) != 0) - (trim ? 1 : 0);
    }
    const int64_t cap = bsdc_toolrec_bytes_bound(n, 4, no, 0, b.nd);
    uint8_t *dst = heap<uint8_t>((size_t)cap);
    int64_t *off = heap<int64_t>((size_t)n + 1);
    expect(bsdc_toolrec_host(&b.o, b.rec.data(), n, b.nd, b.tab.data(), names, 4, cig, no, aux, 0, off, dst, cap) == 0,
           "long cigars");
    expect(off[n] <= cap, "long cigars: total within the bound");
    for (int r = 0; r < n; r++) {
        const uint8_t *p = dst + off[r];
        expect((int64_t)field32(p) + 4 == off[r + 1] - off[r], "long cigars: block_size", r);
        expect((int)(field32(p + 16) & 0xffffu) == nc[r], "long cigars: n_cigar_op", r);
        const int64_t beg = b.o.dump_pos[r], end = beg + reflen[r] - 1;
        const uint32_t bin = field32(p + 12) >> 16;
        if (reflen[r] >= (int64_t)1 << 32) expect(bin == 0, "a reference length past 2^32: bin 0", r);
        else if (beg >> 14 == end >> 14) expect(bin == 4681 + (uint32_t)(beg >> 14), "long cigars: bin", r);
        else if (beg >> 17 == end >> 17) expect(bin == 585 + (uint32_t)(beg >> 17), "long cigars: bin", r);
        else expect(bin < 585, "long cigars: bin", r);
    }
    expect(nc[3 * 6 + 4] == 65535 && nc[3 * 6] == 65533, "the most ops a record holds");
    std::free(names), std::free(aux), std::free(cig), std::free(dst), std::free(off);
}

// 200 records whose table entries share record 0's name (8 bytes), ops (3) and aux bytes (40): the bound counts
// them once, so the records' total passes a destination of exactly the bound.  The heap block is cap bytes long:
// a byte written at or past cap is caught.  The offsets stay whole and every record below cap is complete.
void shared_entries() {
    const int n = 200;
    Batch b(n, 7);
    for (int r = 0; r < n; r++) {
        b.tab[r].name_len = 8, b.tab[r].n_cig = 3, b.tab[r].aux_len = 40;
        b.o.dump_tags[r] = (uint8_t)(r % 16), b.o.dump_pos[r] = (int32_t)(rnd() % (1u << 28));
    }
    uint8_t *names = heap<uint8_t>(8), *aux = heap<uint8_t>(40);
    uint32_t *cig = heap<uint32_t>(3);
    cig[2] = 5u << 4;
    const int64_t cap = bsdc_toolrec_bytes_bound(n, 8, 3, 40, b.nd);
    uint8_t *dst = heap<uint8_t>((size_t)cap);
    int64_t *off = heap<int64_t>((size_t)n + 1);
    expect(bsdc_toolrec_host(&b.o, b.rec.data(), n, b.nd, b.tab.data(), names, 8, cig, 3, aux, 40, off, dst, cap) == 0,
           "shared entries");
    expect(off[n] > cap + 4000, "shared entries: the total passes the bound");
    int whole = 0;
    for (int r = 0; r < n; r++) {
        expect(off[r + 1] - off[r] >= 36 + 9 + 12 + 4 + 7 + 40, "shared entries: a record's size", r);
        if (off[r + 1] > cap) continue;
        whole++;
        expect((int64_t)field32(dst + off[r]) + 4 == off[r + 1] - off[r], "shared entries: block_size", r);
        expect(memcmp(dst + off[r] + 36, names, 8) == 0, "shared entries: name", r);
    }
    expect(whole > 50 && whole < n, "shared entries: cap inside the records");
    std::free(names), std::free(aux), std::free(cig), std::free(dst), std::free(off);
}

void refusals() {
    bsdc_consensus o;
    memset(&o, 0, sizeof o);
    uint8_t *buf = heap<uint8_t>(256);
    int64_t off[2];
    bsdc_toolrec_rec e;
    memset(&e, 0, sizeof e);
    e.name_len = 1;
    o.dump_pos = (int32_t *)buf, o.dump_len = (uint16_t *)buf, o.dump_tags = o.dump_seq = o.dump_qual = buf;
    const uint32_t *u = (const uint32_t *)buf;
    memset(buf, 0, 8);  // (rec[0] and dump_len[0], which share the buffer: slot 0, length 0)
    expect(bsdc_toolrec_host(&o, u, 0, 0, &e, buf, 0, u, 0, buf, 0, off, buf, 0) == 0, "empty batch");
    expect(bsdc_toolrec_host(&o, u, 1, 8, &e, buf, 1, u, 0, buf, 0, off, buf, 256) == 0, "one record");
    expect(bsdc_toolrec_host(nullptr, u, 0, 0, &e, buf, 0, u, 0, buf, 0, off, buf, 0) == BSDC_EINVAL, "null out");
    expect(bsdc_toolrec_host(&o, u, -1, 0, &e, buf, 0, u, 0, buf, 0, off, buf, 0) == BSDC_EINVAL, "negative count");
    expect(bsdc_toolrec_host(&o, u, 1, 8, &e, buf, 1, u, 0, buf, 0, off, buf, 10) == BSDC_EINVAL, "cap below the bound");
    expect(bsdc_toolrec_host(&o, u, 1, 8, &e, buf, 0, u, 0, buf, 0, off, buf, 256) == BSDC_EINVAL, "name leaves names");
    o.dump_seq = nullptr;
    expect(bsdc_toolrec_host(&o, u, 0, 0, &e, buf, 0, u, 0, buf, 0, off, buf, 0) == BSDC_EINVAL, "null dump_seq");
    std::free(buf);
}

}  // namespace

int main() {
    for (int n : {0, 1, 63, 64, 65}) {
        run_case(n, false, false);
        run_case(n, n > 0, false);
        run_case(n, false, true);
    }
    long_cigars();
    shared_entries();
    refusals();
    if (fails) return 1;
    std::printf("toolrec twin ok\n");
    return 0;
}
