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
    refusals();
    if (fails) return 1;
    std::printf("toolrec twin ok\n");
    return 0;
}
