/* Sequential restatement of the GPU BGZF block encoder -- TEST INFRASTRUCTURE ONLY (bgzf_ref.c). */
#ifndef BGZF_REF_H
#define BGZF_REF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* Which paths of the encoder one block took (tests/bgzf_inputs.py builds inputs that must reach
 * them; oracle.py BGZF_STATS names the fields in this order). */
typedef struct {
    int32_t retries_litlen, retries_dist, retries_codelen; /* length-limit retries of the three Huffman builds */
    int32_t literals, matches;                             /* tokens */
    int32_t min_len, max_len, min_dist, max_dist;          /* over the matches (0: none) */
    int32_t clipped;          /* matches that end at their segment's end, shorter than 258 */
    int32_t nice_stops;       /* token searches ended by a match of kNice */
    int32_t lazy_deferrals;   /* a literal because the next position's match is longer */
    int32_t lazy_skipped;     /* no look-ahead because the match is kLazy or longer */
    int32_t cand_round, cand_table; /* candidates from the position's own round / from the hash table */
    int32_t collisions;       /* table candidates whose 4 bytes differ from the position's */
    int32_t chain_cut_kchain, chain_cut_maxdist; /* token searches whose chain went on past kChain / kMaxDist */
    int32_t hlit, hdist, hclen;
    int32_t dist_used;        /* a distance code is used (0: the dl[0] = 1 path) */
    int32_t dist_single;      /* the distance alphabet has one used symbol (the nl == 1 path) */
} bgzf_ref_stats;
int bgzf_ref_block(const uint8_t *in, int n, uint8_t *out);
int bgzf_ref_block_stats(const uint8_t *in, int n, uint8_t *out, bgzf_ref_stats *stats);
void bgzf_huffman_lengths(const uint32_t *freq, int n, int limit, uint8_t *len);
void bgzf_canonical_codes(const uint8_t *len, int n, uint16_t *code);
int bgzf_rle_lengths(const uint8_t *lens, int n, uint8_t *sym, uint8_t *ext);
#ifdef __cplusplus
}
#endif
#endif
