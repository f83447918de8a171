// Stand-alone run of bsdc_bgzf_inflate_host (csrc/bsdc_inflate.hip: the functions the inflate kernel
// shares with its host twin -- the bit reader, the headers, the checks before each copy) for a
// sanitizer build, on the CPU, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//       tests/sanitize/inflate_twin_main.cpp bsseqconsensusreads_amd/csrc/bsdc_inflate.hip -o inflate_twin_asan
//   ./inflate_twin_asan BLOCKS RESULT
// BLOCKS (tests/test_inflate_edges.py writes it): int64 count, n_comp, n_out; count descriptors
// (bsdc_inflate_block); n_comp compressed bytes.  `comp` and `out` live in heap buffers of exactly
// n_comp and n_out bytes, so a read or write one byte outside either is reported.  RESULT: count
// int32 statuses, then the n_out bytes of `out` (0xA5 where nothing was written).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bsdc.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t head[3];
    if (fread(head, sizeof head, 1, f) != 1) return 4;
    const int64_t n = head[0], n_comp = head[1], n_out = head[2];
    if (n <= 0 || n_comp <= 0 || n_out <= 0) return 4;
    bsdc_inflate_block *blk = (bsdc_inflate_block *)malloc((size_t)n * sizeof *blk);
    uint8_t *comp = (uint8_t *)malloc((size_t)n_comp), *out = (uint8_t *)malloc((size_t)n_out);
    int32_t *status = (int32_t *)malloc((size_t)n * sizeof *status);
    if (!blk || !comp || !out || !status) return 5;
    if (fread(blk, sizeof *blk, (size_t)n, f) != (size_t)n || fread(comp, 1, (size_t)n_comp, f) != (size_t)n_comp) return 4;
    fclose(f);
    memset(out, 0xA5, (size_t)n_out);
    for (int64_t i = 0; i < n; i++) status[i] = -1;
    if (bsdc_bgzf_inflate_host(comp, n_comp, blk, n, out, n_out, status) != 0) return 6;
    f = fopen(argv[2], "wb");
    if (!f) return 7;
    if (fwrite(status, sizeof *status, (size_t)n, f) != (size_t)n || fwrite(out, 1, (size_t)n_out, f) != (size_t)n_out) return 7;
    if (fclose(f) != 0) return 7;
    free(status);
    free(out);
    free(comp);
    free(blk);
    puts("inflate_twin ok");
    return 0;
}
