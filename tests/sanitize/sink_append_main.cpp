// Stand-alone check of bsdc_bgzf_sink_append / bsdc_bgzf_sink_take_tail (include/bsdc_io.h) for a
// sanitizer build, on the CPU, from the repository root (DESIGN.md 8.7 has the same recipe):
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -Iinclude tests/sanitize/sink_append_main.cpp \
//       bsseqconsensusreads_amd/csrc/bsdc_io.cpp bsseqconsensusreads_amd/csrc/bsdc_host.cpp -lz -ldl -o sink_append_asan
//   ./sink_append_asan DIR
// Opens a FASTQ writer, appends 0, 1, 65279, 65280 and 65281 bytes to its sinks, flushes, appends
// again and closes; the files must inflate (zlib) to the appended bytes.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bsdc_io.h"

static std::vector<uint8_t> gunzip(const std::string &path) {
    std::vector<uint8_t> out;
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return out;
    uint8_t buf[1 << 16];
    int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) out.insert(out.end(), buf, buf + n);
    gzclose(f);
    return out;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string p[2] = {dir + "/sa1.fq.gz", dir + "/sa2.fq.gz"};
    bsdc_fastq_writer *w = nullptr;
    if (bsdc_fastq_writer_open(p[0].c_str(), p[1].c_str(), 4, &w) != 0) return 2;
    std::vector<uint8_t> want[2];
    const int64_t sizes[5] = {0, 1, 65279, 65280, 65281};
    uint32_t x = 12345;
    for (int k = 0; k < 5; k++) {
        for (int d = 0; d < 2; d++) {
            std::vector<uint8_t> b((size_t)sizes[d == 0 ? k : 4 - k]);
            for (auto &v : b) v = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
            if (bsdc_bgzf_sink_append(bsdc_fastq_writer_sink(w, d), b.empty() ? nullptr : b.data(), (int64_t)b.size()) != 0) return 3;
            want[d].insert(want[d].end(), b.begin(), b.end());
        }
        if (k == 2 && bsdc_fastq_writer_flush(w, 2) != 0) return 4;
    }
    if (bsdc_bgzf_sink_append(bsdc_fastq_writer_sink(w, 0), nullptr, 3) == 0) return 5;  // refused, nothing read
    {  // the tail out and back in: the same bytes in the file
        std::vector<uint8_t> t(65536);
        if (bsdc_bgzf_sink_take_tail(bsdc_fastq_writer_sink(w, 1), t.data(), 0) >= 0) return 9;  // too small
        const int64_t n = bsdc_bgzf_sink_take_tail(bsdc_fastq_writer_sink(w, 1), t.data(), (int64_t)t.size());
        if (n <= 0 || bsdc_bgzf_sink_append(bsdc_fastq_writer_sink(w, 1), t.data(), n) != 0) return 10;
    }
    if (bsdc_fastq_writer_close(w, 2) != 0) return 6;
    for (int d = 0; d < 2; d++)
        if (gunzip(p[d]) != want[d]) return 7 + d;
    for (int d = 0; d < 2; d++) remove(p[d].c_str());
    puts("sink_append ok");
    return 0;
}
