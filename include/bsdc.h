/* bsdc.h -- C-ABI of libbsdc, the MI355X (gfx950) step-5 duplex path.
 *
 * The reference has no plugin API: its boundary is the file contract of the four Snakemake rules
 * convert_Bstrain -> extend -> groupsort_convert -> callduplex (main.snake.py:121-164).  Each entry
 * point below replaces one piece of that contract; INTEGRATION.md shows the ctypes binding the
 * Python host (bsseqconsensusreads_amd/_lib.py) uses, which is also what a maintainer of the
 * reference would add in place of the `python3 tools/...` / `fgbio ...` shell lines.
 *
 *   bsdc_convert      replaces tools/1.convert_AG_to_CT.py:69-186 (per-record B-strand conversion)
 *   bsdc_extend       replaces tools/2.extend_gap.py:112-140       (4-record gap extension)
 *   bsdc_duplex_call  replaces main.snake.py:155-164 fgbio CallDuplexConsensusReads (and, with
 *                     BSDC_MODE_CONVERT|BSDC_MODE_EXTEND in `mode`, the two tools in front of it)
 *   bsdc_filter       replaces fgbio FilterConsensusReads, which the user runs on the unfiltered
 *                     consensus before main.snake.py:70-80 (consensus_to_fq) can read its input
 *
 * Conventions: every function returns 0 on success and a negative errno-style code on failure
 * (message via bsdc_last_error).  Batch and output pointers are DEVICE pointers owned by the
 * caller; work is enqueued on `stream` (a hipStream_t, NULL = the null stream) and is
 * asynchronous: the bucket dispatches fan out over four context-owned side streams after an
 * event on `stream`, and `stream` waits for all of them before any later work on it runs.  The
 * reference genome is copied into library-owned device memory.  One context per GPU per host
 * thread; no global mutable state.  Output order == input family order.
 */
#ifndef BSDC_H
#define BSDC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BSDC_ABI_VERSION 19
#define BSDC_SMALL_BUCKETS 8
#define BSDC_LARGE_BUCKETS 6
#define BSDC_LARGE_LDS_MAX 158912 /* LDS arena bytes one large-family workgroup may use */ /* LDS arena size classes of the wavefront-per-family kernel */

#define BSDC_EINVAL (-22)
#define BSDC_ENOMEM (-12)
#define BSDC_EDEVICE (-5)

/* fgbio CallDuplexConsensusReads flags as the pipeline passes them (main.snake.py:163).
 *
 * Supported domain -- bsdc_ctx_create and bsdc_ctx_set_params return BSDC_EINVAL outside it, with
 * the reason in bsdc_last_error (of the context; bsdc_last_error(NULL) after a failed create):
 *   error_rate_pre_umi   1.25 <= pre < 46.999.  A consensus quality reaches floor(pre + 0.001), and
 *                        the vote's agreement-case table (dthr, 48 entries, read at Q + 1) covers
 *                        qualities up to 46.  The pipeline passes 45.
 *   error_rate_post_umi  0 < post <= 1000.
 *   min_input_base_quality  only 0: no kernel masks input bases, so another value is refused
 *                        instead of being ignored.
 *   min_reads            only 0.
 *   min_consensus_base_quality  0..94 (94: every single-strand column is (N, 2)).
 * Quality bytes are unsigned phred values 0..255 everywhere (overlap consensus, vote: lr has 256
 * entries): a byte above 93, BAM's "missing quality" 0xFF included, is that phred and not a
 * marker; only results are capped at 93. */
typedef struct {
    double error_rate_pre_umi;                /* --error-rate-pre-umi=45 */
    double error_rate_post_umi;               /* --error-rate-post-umi=30 */
    int32_t min_input_base_quality;           /* --min-input-base-quality=0 (only 0 is supported) */
    int32_t consensus_call_overlapping_bases; /* --consensus-call-overlapping-bases=true */
    int32_t min_reads;                        /* --min-reads=0 (only 0 is supported) */
    int32_t min_consensus_base_quality;       /* single-strand calls with Q below it -> (N, 2), 0..94:
                                                 2 for step 5 (fgbio DuplexConsensusCaller's single-strand
                                                 caller masks at PhredScore.MinValue; main.snake.py:163
                                                 passes no such flag), 0 for step 1
                                                 (--min-consensus-base-quality=0, main.snake.py:54) */
} bsdc_params;

/* Per-record `link` word (host-built) */
#define BSDC_LINK_MATE_MASK 0xFFFFu   /* template mate (R2 of this R1) index within family; 0xFFFF = none */
#define BSDC_MAX_FAMILY_RECORDS 65534 /* so every in-family index stays below 0xFFFF; the host planner
                                         (bsdc_materialize_prepare, batch.materialize_py) refuses larger families */
/* The alignment filter keeps each source read's simplified cigar at a 16-bit offset into the
   family's slots (one per M-only record, ops + 2 per complex record), so a family that holds a
   complex cigar has at most this many: every offset is then below 65536.  The host planner
   refuses a larger one, as above. */
#define BSDC_MAX_FILTER_SLOTS 65536
#define BSDC_LINK_AB (1u << 16)       /* MI ends in /A */
#define BSDC_LINK_BA (1u << 17)       /* MI ends in /B */
#define BSDC_LINK_COMPLEX (1u << 18)  /* cigar is not a single M-like run: read cig_* */
#define BSDC_LINK_RT (1u << 19)       /* read-through trim candidate: read rt[] */
#define BSDC_LINK_CONVERT (1u << 20)  /* tool 1 converts this record (flag 1/83/163) */
#define BSDC_LINK_EXT_RIGHT (1u << 21) /* tool 2: gets the partner's first base prepended */
#define BSDC_LINK_EXT_LEFT (1u << 22) /* tool 2: gets the partner's last base appended if RD=1 */
#define BSDC_LINK_PARTNER_SHIFT 23    /* 2 bits: tool-2 partner index within the family */
#define BSDC_LINK_RD_IN (1u << 25)    /* RD tag of an already-converted input (extend-only mode) */
#define BSDC_LINK_USABLE (1u << 26)   /* paired primary record with an /A or /B MI */

/* A batch of MI families in HBM, structure-of-arrays.  Record r of family f is
 * fam_off[f] <= r < fam_off[f+1].  Records live in "slots": slot r starts at nibble/byte index
 * S = rec[4r] of `seq` (nt16 codes "=ACMGRSVTWYHKDBN", two per byte, high nibble first, as in
 * BAM) and of `qual`, is round4(len+2) long, and holds the record's bases/quals at S+1 .. S+len
 * (S+0 and S+len+1 are the prepend / append room of tools 1 and 2).  A family's slots are
 * contiguous and its first slot starts at a multiple of 32.  Soft clips are already stripped by
 * the host (tools 1 and 2 both strip them before anything else). */
typedef struct {
    int64_t n_rec;
    int64_t n_fam;
    const uint32_t *fam_off;     /* [n_fam+1] */
    const uint32_t *rec;         /* [4*n_rec] slot start, pos (int32, 0-based), len | flag << 16, link */
    const uint32_t *rec_win;     /* [2*n_rec] converted records: reference window start nibble
                                    (= contig start + max(pos-1,0)), valid nibbles (<= len+2) */
    const uint32_t *cig_off;     /* [n_rec]   complex records only: first op in `cigar` */
    const uint32_t *cig_info;    /* [n_rec]   complex only: n_ops | reflen << 16 */
    const uint32_t *cigar;       /*           BAM-encoded ops (soft/hard clips removed) */
    const int32_t *rt;           /* [4*n_rec] RT records only: next_pos, tlen, mate unclipped start, end */
    const uint8_t *seq;
    const uint8_t *qual;
    const uint32_t *small_fams;  /* families processed one wavefront each, BSDC_SMALL_BUCKETS consecutive buckets;
                                    4 words per family: family, first record,
                                    n_rec | (image bytes / 32) << 8, image base (first slot) */
    int64_t n_small[BSDC_SMALL_BUCKETS];      /* families per bucket */
    int32_t small_arena[BSDC_SMALL_BUCKETS];  /* LDS bytes per wavefront of each bucket (multiple of 16) */
    const uint32_t *large_fams;  /* families processed one workgroup each, BSDC_LARGE_BUCKETS consecutive
                                    buckets; 4 words per family: family, first record, n_rec,
                                    image bytes (from the first slot) */
    int64_t n_large[BSDC_LARGE_BUCKETS];      /* families per bucket */
    int32_t large_arena[BSDC_LARGE_BUCKETS];  /* bytes per workgroup of each bucket (multiple of 16); a
                                                 bucket beyond BSDC_LARGE_LDS_MAX keeps its arenas in `scratch` */
    int32_t max_len;             /* max record length */
    int32_t split_part_arena;    /* LDS bytes per part workgroup (256 threads) */
    /* Part mode (k_large): a family beyond the LDS buckets whose records hold no complex cigar and
     * no tool-2 role is cut into parts of whole templates that each fit split_part_arena; a part
     * runs everything up to the vote in LDS and leaves its per-column likelihood sums and read
     * counts in `scratch`; one workgroup per family then adds the parts up, calls, combines and
     * writes (a near-tie column -- rare -- makes that family run whole in its HBM arena instead). */
    const uint32_t *split_parts; /* 4 words per part: family, first part record, n_rec (< 256) | its row in
                                    split_fams << 8, image bytes */
    int64_t n_split_parts;
    const uint32_t *split_part_recs; /* 4 words per part record: batch record, slot in the part's image,
                                        part-local index of its mate (0xFFFF: none) | record length << 16,
                                        slot in the batch image */
    const uint32_t *split_fams;  /* 8 words per family: family, first record, n_rec, image bytes, first part,
                                    parts, fallback arena offset in scratch / 16, fallback arena bytes */
    int64_t n_split_fams;
    int64_t split_partial_off;   /* scratch offset of the parts' sums: [part][8] int32 (set reads, set
                                    lengths), then [part][4][stride] int32x4 sums (slot k: the set's
                                    k-th multi-base column), [part][4][stride] u8x4 counts (without
                                    BSDC_MODE_TAGS: the region's first [part][4][stride] bytes hold
                                    the columns' ORs of one-hot A/C/G/T codes instead), [part][4][stride]
                                    int32 one-base sums (a multi-base column: its sums' slot k) */
} bsdc_family_batch;

/* Outputs (device pointers).  Consensus slot (f, end) holds `stride` bases. */
typedef struct {
    int32_t stride;              /* >= max_len + 2, multiple of 16 */
    int32_t reserved;
    uint8_t *status;             /* [n_fam] bit0 pair emitted, bit1 AB strand used, bit2 BA strand used */
    uint16_t *len;               /* [2*n_fam] R1, R2 lengths */
    uint8_t *seq;                /* [2*n_fam*stride/2] packed nt16 */
    uint8_t *qual;               /* [2*n_fam*stride] */
    /* optional stage dump (NULL = off): the records after tool 1 + tool 2 */
    int32_t *dump_pos;           /* [n_rec] */
    uint16_t *dump_len;          /* [n_rec] */
    uint8_t *dump_tags;          /* [n_rec] bit0 RD=1, bit1 LA present, bit2 prepended M, bit3 appended M */
    uint8_t *dump_seq;           /* [slot start + j] one nt16 code per byte */
    uint8_t *dump_qual;
    uint8_t *scratch;            /* arenas of the large buckets beyond BSDC_LARGE_LDS_MAX, one region per
                                    bucket (their dispatches may run concurrently): the sum of
                                    n_large[q] * large_arena[q] over those buckets; then the split
                                    families' fallback arenas and the parts' sums (bsdc_family_batch);
                                    + 256 bytes */
    /* optional single-strand consensus reads and their per-column statistics (BSDC_MODE_TAGS),
     * the inputs of fgbio's per-read / per-base consensus tags (aD/aM/aE, ad/ae/ac/aq, ...;
     * cD/cM/cE, cd/ce for the molecular caller).  Row (f, s), s = 0 AB-R1, 1 AB-R2, 2 BA-R1,
     * 3 BA-R2, holds `stride` columns of family f's set s (sequencing orientation). */
    uint16_t *ss_len;            /* [4*n_fam] single-strand consensus length (0 = set empty) */
    uint8_t *ss_base;            /* [4*n_fam*stride] nt16 code per byte (N when Q < 2) */
    uint8_t *ss_qual;            /* [4*n_fam*stride] */
    uint8_t *ss_depth;           /* [4*n_fam*stride] reads with an A/C/G/T at the column (ABI 14: u8,
                                    saturated at 255; exact in ss_wdepth for a family with a wide row) */
    uint8_t *ss_err;             /* [4*n_fam*stride] depth - reads showing the raw (pre-mask) best base (u8,
                                    saturated; exact in ss_werr) */
    /* (ABI 14) families of more than 255 records, whose depths may not fit a byte: ss_wide[f] = the
     * family's wide row w (-1: none; the host numbers them), and rows (w, s) of ss_wdepth / ss_werr
     * hold its exact depths / errors, u16 saturated at 32767 as fgbio's tags.  NULL with no such
     * family.  (A family routed to the small kernels has at most 64 records.) */
    const int32_t *ss_wide;      /* [n_fam] */
    uint16_t *ss_wdepth;         /* [4*n_wide*stride] */
    uint16_t *ss_werr;           /* [4*n_wide*stride] */
} bsdc_consensus;

#define BSDC_MODE_CONVERT 1
#define BSDC_MODE_EXTEND 2
#define BSDC_MODE_VOTE 4
#define BSDC_MODE_DUMP 8
#define BSDC_MODE_TAGS 64       /* also write the ss_* outputs (with BSDC_MODE_VOTE) */
#define BSDC_MODE_SKIP_SMALL 16 /* profiling: do not launch the small-family kernel */
#define BSDC_MODE_SKIP_LARGE 32 /* profiling: do not launch the large-family kernel */
#define BSDC_MODE_STOP_SHIFT 8  /* profiling: (mode >> 8) & 15 = k > 0 stops the small kernel after phase k */

typedef struct bsdc_ctx bsdc_ctx;

int32_t bsdc_abi_version(void);
int32_t bsdc_ctx_create(int32_t device, const bsdc_params *params, bsdc_ctx **out);
/* Replace a context's flags (e.g. one GPU context serving both callers: step 1's flags at
 * main.snake.py:54, step 5's at :163).  New error rates rebuild the tables after a device sync. */
int32_t bsdc_ctx_set_params(bsdc_ctx *ctx, const bsdc_params *params);
void bsdc_ctx_destroy(bsdc_ctx *ctx);
const char *bsdc_last_error(const bsdc_ctx *ctx);

/* Reference genome, host pointers: nt16 codes of the upper-cased FASTA, packed two per byte;
 * contig_off[tid] = first nibble of contig tid (-1 = contig absent from the FASTA).  Batches
 * address it through rec_win, which the host derives from the same contig table. */
int32_t bsdc_load_reference(bsdc_ctx *ctx, const uint8_t *packed_nt16, int64_t n_nibbles,
                            const int64_t *contig_off, const int64_t *contig_len, int32_t n_contig);

/* The one launcher.  mode = OR of BSDC_MODE_*. */
int32_t bsdc_run(bsdc_ctx *ctx, const bsdc_family_batch *batch, bsdc_consensus *out, int32_t mode,
                 void *stream);

/* Named entry points of the three reference stages (== bsdc_run with a fixed mode). */
int32_t bsdc_convert(bsdc_ctx *ctx, const bsdc_family_batch *batch, bsdc_consensus *out, void *stream);
int32_t bsdc_extend(bsdc_ctx *ctx, const bsdc_family_batch *batch, bsdc_consensus *out, void *stream);
int32_t bsdc_duplex_call(bsdc_ctx *ctx, const bsdc_family_batch *batch, bsdc_consensus *out,
                         int32_t with_tools, void *stream);

/* Arena bytes one family needs (host-side helpers shared with the batch builder):
 * workgroup kernel (slot_bytes = 2 x the family's image bytes) and wavefront kernel (img = slot
 * span rounded to 32, n_conv = converted records, max_len = the batch's max record length). */
int64_t bsdc_family_arena_bytes(int32_t n_rec, int64_t slot_bytes, int32_t max_len, int64_t complex_ops);
int64_t bsdc_small_arena_bytes(int32_t n_rec, int64_t img, int32_t n_conv, int64_t complex_ops, int32_t max_len);

/* The likelihood tables the vote kernel uses (host copies), for cross-checks. */
int32_t bsdc_get_tables(const bsdc_ctx *ctx, int64_t *lr256, float *thresh94);
/* Same tables for given error rates, without a context (no GPU needed). */
void bsdc_model_tables(double error_rate_pre_umi, double error_rate_post_umi, int64_t *lr256, float *thresh94);
/* The near-tie tables: fgbio's per-read log-space terms in double precision,
   ln P(correct) and ln P(error) / 3 per phred, which a near-tie column sums in fgbio's read order. */
void bsdc_model_tables_fp64(double error_rate_pre_umi, double error_rate_post_umi, double *lnc256, double *lne3_256);
/* The vote's agreement-case tables: Q(D) = qlo[D >> 16] + (D >= dthr[qlo[D >> 16] + 1]).
   The table helpers here are unchecked: they tabulate any rates, also ones bsdc_ctx_create refuses
   (for which dthr's 48 entries do not cover every reachable Q). */
void bsdc_agree_tables(double error_rate_pre_umi, double error_rate_post_umi, uint8_t *qlo2048, int32_t *dthr48);
/* The general case's phred buckets: Q(S) = the largest k >= sq[j] with S <= thresh[k], j = the
   bucket of S ((float bits >> 21) - ((127 - 32) << 2), clamped to [0, 135]). */
void bsdc_phred_buckets(double error_rate_pre_umi, double error_rate_post_umi, uint8_t *sq144);

/* BGZF compression of the output BAM on the GPU (replaces the deflate of fgbio's / htsjdk's BAM
   writer behind CallDuplexConsensusReads --output, main.snake.py:159-163; csrc/bsdc_bgzf.hip):
   device bytes in[0, n) as blocks of 65280 bytes, one dynamic-Huffman DEFLATE block each.
   bsdc_bgzf_deflate compresses blocks blk0 .. blk0 + nblk - 1 into the scratch
   (bsdc_bgzf_scratch_bytes(nblk) bytes) and writes sizes[blk0 + b]: the BGZF block size, its
   CRC32 / ISIZE trailer counted but left to the host (libbsdc_io bsdc_bgzf_sink_put), or
   0 when the block does not fit (the host deflates it).  bsdc_bgzf_pack then copies block b's
   bytes from the scratch to out + (sizes[0] + .. + sizes[blk0 + b - 1]), so successive launches
   over one stream's blocks pack them back to back with no host round trip.  Device pointers;
   stream = hipStream_t. */
int64_t bsdc_bgzf_scratch_bytes(int64_t max_blocks);

/* Page-lock a caller's host range for DMA (hipHostRegister) / release it: a multi-GPU worker's
 * mappings of the shared segments its batches and outputs travel in (fleet.py), so uploads and
 * fetches run by DMA from / into them.  0, or BSDC_EDEVICE with the runtime's error cleared (a
 * range that stays pageable still works, at the pageable copy rate).  No reference counterpart:
 * the reference runs step 5 as one process per rule (main.snake.py:121-164, fgbio --threads). */
int32_t bsdc_host_register(int32_t device, void *ptr, int64_t nbytes);
int32_t bsdc_host_unregister(int32_t device, void *ptr);
int32_t bsdc_bgzf_deflate(const uint8_t *in, int64_t n, int64_t blk0, int64_t nblk, uint8_t *scratch,
                          int32_t *sizes, void *stream);
int32_t bsdc_bgzf_pack(const uint8_t *scratch, const int32_t *sizes, int64_t blk0, int64_t nblk, uint8_t *out,
                       void *stream);

/* fgbio FilterConsensusReads on the device (the step every user of the unfiltered consensus runs
 * next: the reference's consensus_to_fq rule, main.snake.py:70-80, reads a _molecular_filtered.bam),
 * from the single-strand rows a BSDC_MODE_TAGS run left in HBM; rules in DESIGN.md section 3.8
 * (restated from fgbio: PARITY UNPINNED).  The three-entry fields are ordered duplex ("cc"), AB,
 * BA, as fgbio's one-to-three-valued flags.
 * Supported domain (BSDC_EINVAL outside it, the message names the field): min_reads >= 0 and
 * non-increasing; every rate and max_no_call_fraction in [0, 1]; min_base_quality 0..93;
 * min_mean_base_quality -1..93. */
typedef struct {
    int32_t min_reads[3];               /* -M */
    double max_read_error_rate[3];      /* -E (fgbio's default 0.025) */
    double max_base_error_rate[3];      /* -e (0.1) */
    int32_t min_base_quality;           /* -N: consensus bases below it become (N, 2) */
    double max_no_call_fraction;        /* -n (0.2) */
    int32_t min_mean_base_quality;      /* -q; -1 = off */
    int32_t require_single_strand_agreement; /* -s */
} bsdc_filter_params;

#define BSDC_FILT_MINREADS 1  /* bsdc_filter's reason bits */
#define BSDC_FILT_READERR 2
#define BSDC_FILT_NOCALL 4
#define BSDC_FILT_MEANQ 8

/* Enqueued on the stream of the bsdc_run(.. | BSDC_MODE_TAGS) that filled `out`, after it.  kind: 0
 * duplex (step 5), 1 molecular (step 1: rows 0 / 1 are R1 / R2, no BA side).  filt[f] = 0 for a
 * family kept or not emitted, else the OR of the reason bits of its two ends; masked[2f + e] = the
 * columns of end e newly masked to (N, 2); out->seq and out->qual are rewritten in place (an end
 * that passed the read-level gate is masked even if the other end drops the template).  out->status
 * and the ss_* rows are only read.  Device pointers; BSDC_EINVAL when out->ss_* are NULL. */
int32_t bsdc_filter(bsdc_ctx *ctx, const bsdc_filter_params *params, int32_t kind, int64_t n_fam,
                    bsdc_consensus *out, uint8_t *filt, uint16_t *masked, void *stream);

/* (ABI 17) Inflate of the input BAM's BGZF blocks on the GPU (replaces the inflate of htsjdk's BAM
 * reader behind CallDuplexConsensusReads --input, main.snake.py:157-163; csrc/bsdc_inflate.hip):
 * block b's raw DEFLATE data comp[src, src + clen) -> its isize bytes at out + dst, one workgroup
 * per block; status[b] = 0 when the block inflated to exactly isize bytes, else one of the codes
 * below and nothing of the block is written.  The input is untrusted: the kernel reads `comp`
 * only inside [src, src + clen), writes `out` only inside [dst, dst + isize), and ends on any
 * bytes.  CRC32 / ISIZE stay with the host (libbsdc_io checks the returned
 * bytes).  bsdc_bgzf_inflate: device pointers, enqueued on `stream` (hipStream_t); returns 0 once
 * launched.  bsdc_bgzf_inflate_host: host pointers, the same decoding functions run sequentially
 * on the CPU (no GPU needed) -- the twin the corrupt-input tests run first. */
typedef struct {
    int64_t src;    /* offset of the block's raw deflate data in comp */
    int32_t clen;   /* its bytes */
    int32_t isize;  /* the bytes it inflates to (BGZF ISIZE, <= 65536) */
    int64_t dst;    /* offset of the block's bytes in out */
} bsdc_inflate_block;

#define BSDC_INFLATE_EBTYPE 1     /* block type 3 */
#define BSDC_INFLATE_ESTORED 2    /* stored block: LEN != ~NLEN */
#define BSDC_INFLATE_ELENGTHS 3   /* over-subscribed or incomplete code lengths (zlib's rules) */
#define BSDC_INFLATE_EREPEAT 4    /* repeat code with no previous length, or running past HLIT + HDIST */
#define BSDC_INFLATE_ESYMBOL 5    /* literal/length symbol 286 / 287 or distance symbol 30 / 31 */
#define BSDC_INFLATE_EDIST 6      /* distance reaching before the block's start */
#define BSDC_INFLATE_EOVERFLOW 7  /* output would exceed isize */
#define BSDC_INFLATE_ESHORT 8     /* final end of block before isize bytes */
#define BSDC_INFLATE_EINPUT 9     /* the clen bytes are exhausted */
#define BSDC_INFLATE_ECOUNTS 10   /* HLIT > 286 or HDIST > 30 */
#define BSDC_INFLATE_ENOEOB 11    /* a dynamic block without an end-of-block code */
#define BSDC_INFLATE_ECODE 12     /* bits that are no code of an incomplete (or empty) code */
#define BSDC_INFLATE_ERANGE 13    /* the descriptor leaves comp / out, isize > 65536, or clen > 16 MiB */

int32_t bsdc_bgzf_inflate(const uint8_t *comp, int64_t n_comp, const bsdc_inflate_block *blk, int64_t nblk,
                          uint8_t *out, int64_t n_out, int32_t *status, void *stream);
int32_t bsdc_bgzf_inflate_host(const uint8_t *comp, int64_t n_comp, const bsdc_inflate_block *blk, int64_t nblk,
                               uint8_t *out, int64_t n_out, int32_t *status);

/* (ABI 18) The FASTQ pair formatted on the device (replaces picard SamToFastq behind the rules
 * consensus_to_fq / consensusduplex_to_fq, main.snake.py:58-67,167-177, and the host writer's text
 * pass; csrc/bsdc_fastq.hip): the text of a batch's kept families from the consensus where the vote
 * left it.  `out` is the bsdc_consensus the vote filled (status, len, seq, qual, stride; qual 4-byte
 * aligned) and filt the filter's output or NULL: family f is written when status[f] & 1 and (filt
 * NULL or filt[f] == 0).  name_off [n_fam + 1] / name_buf: a packed table, one name per family (the
 * "prefix:MI" of the BAM's records), at most 254 bytes each; name_off_host is the caller's host
 * copy of name_off, which is what gets checked.  Per file d = 0 (first of pair), 1 (second):
 * off_d [n_fam + 1] receives the exclusive prefix sum of the families' byte counts (off_d[n_fam] =
 * the total) and text_d + off_d[f] the bytes of family f,
 *   '@' name '/' ('1' | '2') '\n' SEQ '\n' '+' '\n' QUAL '\n'     (8 + name + 2 * len[2f + d] bytes)
 * SEQ = row (f, d) of out->seq through "=ACMGRSVTWYHKDBN" (high nibble first), QUAL = (uint8_t)(33 + q).
 * No byte at or past text_d + cap_d is written; the totals are true whatever the caps, so the
 * caller compares.  bsdc_fastq_text_bound = a size known before the launch: the sum over the
 * families of 8 + name length, plus 2 * n_fam * stride.  tmp: bsdc_fastq_tmp_bytes of 8-byte
 * aligned scratch.  Sizes, scan and text are enqueued on `stream` (hipStream_t) by the one call,
 * after the vote and the filter on it; device pointers but for `out` itself and name_off_host.
 * BSDC_EINVAL: a NULL pointer (filt apart), a negative count or cap, a name outside 0..254 bytes. */
int64_t bsdc_fastq_text_bound(int64_t n_fam, int64_t name_bytes, int32_t stride);
int64_t bsdc_fastq_tmp_bytes(int64_t n_fam);
int32_t bsdc_fastq_format(const bsdc_consensus *out, const uint8_t *filt, int64_t n_fam, const int64_t *name_off,
                          const uint8_t *name_buf, const int64_t *name_off_host, int64_t *off0, int64_t *off1,
                          uint8_t *text0, uint8_t *text1, int64_t cap0, int64_t cap1, uint8_t *tmp, void *stream);

/* (ABI 18) The CRC32 (zlib / gzip) of whole BGZF blocks on the device (replaces the checksum pass of
 * the gzip writer behind the same rules' F= / F2= outputs, main.snake.py:58-67,167-177):
 * crc[blk0 + b] = the CRC32 of in[(blk0 + b) * 65280, + 65280) for b < nblk, one workgroup per
 * block; what bsdc_bgzf_sink_put of libbsdc_io takes as the blocks' crc[].  A file's short last
 * block stays with the host.  Device pointers, `in` 16-byte aligned; enqueued on `stream`. */
int32_t bsdc_bgzf_crc32(const uint8_t *in, int64_t blk0, int64_t nblk, uint32_t *crc, void *stream);

/* (ABI 19) The output BAM's records written on the device (replaces the record encoder of fgbio's /
 * htsjdk's BAM writer behind CallDuplexConsensusReads / CallMolecularConsensusReads --output,
 * main.snake.py:46-55,155-164, and the host writer's tag and encode passes; csrc/bsdc_bam.hip,
 * DESIGN.md section 8.8).  `out` is the bsdc_consensus the vote filled (seq, qual and, with_tags,
 * the ss_* rows 4-byte aligned) and filt the filter's output or NULL: family f is written when
 * status[f] & 1 and (filt NULL or filt[f] == 0).  kind: 0 duplex, 1 molecular, as bsdc_filter's.
 * name_off / name_buf and aux_off / aux_buf: packed tables [n_fam + 1], one read name (at most 253
 * bytes) and one run of aux bytes (RG / MI / RX, both mates alike; at most 1 MiB) per family; the
 * *_host arguments are the caller's host copies of the offsets, which are what gets checked.
 * off [n_fam + 1] receives the exclusive prefix sum of the families' byte counts (off[n_fam] = the
 * total, true whatever cap is) and rec + off[f] the family's records R1, R2, each what libbsdc_io
 * encodes for it: block_size; tid -1, pos -1, l_read_name, mapq 0, bin 4680, no cigar, flag 77 /
 * 141, l_seq = len[2f + e], next -1 / -1, tlen 0; name NUL; (l_seq + 1) / 2 bytes of row (f, e) of
 * out->seq, the pad nibble of an odd length 0; l_seq QUAL bytes; the aux bytes; with_tags the bytes
 * of libbsdc_io's bsdc_consensus_tags for the record (kind 0: cD cM cE aD aM aE [bD bM bE] ad ae ac
 * aq [bd be bc bq]; kind 1: cD cM cE cd ce; rows cut to l_seq; integers in the smallest BAM type;
 * a read without depth gets the 0 / 0 of the host that launches).  No byte at or past rec + cap is
 * written.  bsdc_bam_bytes_bound = a size known before the launch (name_bytes, aux_bytes: the
 * tables' sizes), < 0 on bad arguments; tmp: bsdc_bam_tmp_bytes of 8-byte aligned scratch.
 * Everything is enqueued on `stream` by the one call, after the vote and the filter on it; device
 * pointers but for `out` itself and the two *_host copies.  BSDC_EINVAL, before any device is
 * touched: a NULL pointer (filt apart), a negative count or cap, offsets that go backwards, a name
 * over 253 bytes, with_tags with out->ss_* NULL, kind outside 0 / 1. */
int64_t bsdc_bam_bytes_bound(int64_t n_fam, int64_t name_bytes, int64_t aux_bytes, int32_t stride, int32_t kind,
                             int32_t with_tags);
int64_t bsdc_bam_tmp_bytes(int64_t n_fam);
int32_t bsdc_bam_format(const bsdc_consensus *out, const uint8_t *filt, int32_t kind, int32_t with_tags, int64_t n_fam,
                        const int64_t *name_off, const uint8_t *name_buf, const int64_t *name_off_host,
                        const int64_t *aux_off, const uint8_t *aux_buf, const int64_t *aux_off_host, int64_t *off,
                        uint8_t *rec, int64_t cap, uint8_t *tmp, void *stream);

/* (new exports, ABI 19 still) The family images gathered on the device from the records' SEQ and
 * QUAL bytes as they lie in the BAM (replaces the host's unpack of htsjdk-style record bytes into
 * per-base arrays and their copy into the batch, behind CallDuplexConsensusReads /
 * CallMolecularConsensusReads --input, main.snake.py:46-55,155-164; csrc/bsdc_image.hip, DESIGN.md
 * section 8.9).  raw[0, n_raw): for every record its SEQ field ((l_seq + 1) / 2 bytes, two nt16
 * codes a byte, high nibble first) followed by its QUAL field (l_seq bytes), at any byte offset.
 * One bsdc_image_rec per batch record; the output is the bsdc_family_batch's seq [n_slots / 2] and
 * qual [n_slots]: record bases skip .. skip + len - 1 at nibbles / bytes slot + 1 .. slot + len,
 * every other byte of both images 0 -- the bytes libbsdc_io's bsdc_materialize_fill and
 * bsdc_split_move make from unpacked bases.  n_slots is a multiple of 8; raw, seq_img and qual_img
 * are 4-byte aligned.  bsdc_image_gather: device pointers but for recs_host, the caller's host
 * copy of the table, which is what gets checked; the images are zeroed and filled on `stream`
 * (hipStream_t); returns 0 once enqueued.  BSDC_EINVAL, before anything is enqueued, naming the
 * record and the field (bsdc_last_error of the context; bsdc_image_last_error, thread-local, also
 * without one): src or src + (l_seq + 1) / 2 + l_seq outside [0, n_raw]; skip + len > l_seq or a
 * negative one; slot % 4 != 0; slot + 1 + len > n_slots.  The kernel makes the same test per entry
 * and skips a bad one, and reads and writes inside the three buffers whatever the table holds.
 * bsdc_image_gather_host: host pointers, the same per-dword function run sequentially on the CPU
 * (no GPU needed; ctx may be NULL) -- the twin the tests compare the kernel with. */
typedef struct {
    int64_t src;    /* byte offset of the record's SEQ field in raw; QUAL at src + (l_seq + 1) / 2 */
    int32_t l_seq;  /* the record's length */
    int32_t skip;   /* leading bases dropped (the plan's sL) */
    int32_t len;    /* bases kept (the plan's L) */
    uint32_t slot;  /* the record's batch slot, a multiple of 4 */
} bsdc_image_rec;

int32_t bsdc_image_gather(bsdc_ctx *ctx, const uint8_t *raw, int64_t n_raw, const bsdc_image_rec *recs,
                          const bsdc_image_rec *recs_host, int64_t n_rec, int64_t n_slots, uint8_t *seq_img,
                          uint8_t *qual_img, void *stream);
int32_t bsdc_image_gather_host(bsdc_ctx *ctx, const uint8_t *raw, int64_t n_raw, const bsdc_image_rec *recs,
                               int64_t n_rec, int64_t n_slots, uint8_t *seq_img, uint8_t *qual_img);
const char *bsdc_image_last_error(void);

/* (new exports, ABI 19 still) Per-run consensus metrics reduced on the device (no reference
 * counterpart: a user of the reference histograms the tagged BAM's cD/aD/bD, cE/aE/bE and per-base
 * tags with another tool before choosing FilterConsensusReads' thresholds; csrc/bsdc_metrics.hip,
 * DESIGN.md sections 3.9 and 8.10).  The accumulator is bsdc_metrics_words(cycles) u64 words
 * (BSDC_EINVAL for cycles outside 2..1024), zeroed once by the caller and added to by every call:
 *   [0, 16)  counts: BSDC_METRICS_FAMILIES families seen, _EMITTED those with status & 1, _RECORDS the
 *            output records measured (2 per emitted family that is not skipped), _SKIPPED emitted
 *            families not read (a length beyond the stride, a wide row outside [0, n_wide)); from
 *            bsdc_metrics_filter: _KEPT emitted families with filt == 0, _MINREADS / _READERR /
 *            _NOCALL / _MEANQ emitted families carrying that reason bit, _MASKED the sum of masked;
 *            the other words stay 0
 *   BSDC_METRICS_DEPTH_HIST  [3][2][256]  [kind cD / aD / bD][end][min(D, 255)], one per record (an
 *            absent b counts at 0)
 *   BSDC_METRICS_RATE_HIST   [3][2][102]  [kind cE / aE / bE][end][bin], bin = min((int)floor((double)xE
 *            * 1000.0), 100), an infinite rate 100, NaN 101 (an absent b counts at 0)
 *   BSDC_METRICS_QUAL_HIST   [2][95]      [end][consensus quality, capped at 93] of every non-N column
 *            inside the length; bin 94 = the N columns
 *   BSDC_METRICS_BY_CYCLE    [2][cycles][6]  [end][min(column, cycles - 1)]: records covering the column,
 *            no-calls, sum of consensus quality, sum of depth ad + bd, sum of strand errors ae + be,
 *            disagreements (both rows present, both codes A/C/G/T, different)
 * The views a / b, the rows' cut to the consensus length and the per-read values are bsdc_filter's
 * (DESIGN.md 3.8).  bsdc_metrics reads `out` as the vote left it, so it is enqueued on the vote's
 * stream after it and BEFORE bsdc_filter masks seq / qual: the histograms describe the unfiltered
 * consensus.  n_wide = the rows of out->ss_wdepth / ss_werr (0 with none); molecular as bsdc_filter's
 * kind.  bsdc_metrics_filter adds the filter's outcome, after bsdc_filter on the same stream.  Device
 * pointers but for `out` itself; acc 8-byte aligned, the rows 4-byte aligned.  The *_host twins take
 * host pointers and run the same per-record function sequentially on the CPU (no GPU needed; ctx
 * may be NULL).  BSDC_EINVAL, before anything is enqueued, naming the field (bsdc_last_error of the
 * context; bsdc_metrics_last_error, thread-local, also without one): a NULL buffer (ss_wide apart),
 * cycles outside 2..1024, a stride that is no positive multiple of 16, a negative count, molecular
 * outside 0..1. */
#define BSDC_METRICS_FAMILIES 0
#define BSDC_METRICS_EMITTED 1
#define BSDC_METRICS_RECORDS 2
#define BSDC_METRICS_SKIPPED 3
#define BSDC_METRICS_KEPT 4
#define BSDC_METRICS_MINREADS 5
#define BSDC_METRICS_READERR 6
#define BSDC_METRICS_NOCALL 7
#define BSDC_METRICS_MEANQ 8
#define BSDC_METRICS_MASKED 9
#define BSDC_METRICS_DEPTH_HIST 16
#define BSDC_METRICS_RATE_HIST (16 + 3 * 2 * 256)
#define BSDC_METRICS_QUAL_HIST (BSDC_METRICS_RATE_HIST + 3 * 2 * 102)
#define BSDC_METRICS_BY_CYCLE (BSDC_METRICS_QUAL_HIST + 2 * 95)

int64_t bsdc_metrics_words(int32_t cycles);
int32_t bsdc_metrics(bsdc_ctx *ctx, const bsdc_consensus *out, int64_t n_fam, int64_t n_wide, int32_t molecular,
                     int32_t cycles, uint64_t *acc, void *stream);
int32_t bsdc_metrics_filter(bsdc_ctx *ctx, const uint8_t *status, const uint8_t *filt, const uint16_t *masked,
                            int64_t n_fam, uint64_t *acc, void *stream);
int32_t bsdc_metrics_host(bsdc_ctx *ctx, const bsdc_consensus *out, int64_t n_fam, int64_t n_wide, int32_t molecular,
                          int32_t cycles, uint64_t *acc);
int32_t bsdc_metrics_filter_host(bsdc_ctx *ctx, const uint8_t *status, const uint8_t *filt, const uint16_t *masked,
                                 int64_t n_fam, uint64_t *acc);
const char *bsdc_metrics_last_error(void);

/* (new exports, ABI 19 still) The records after tool 1 and tool 2 written on the device as BAM
 * records (replaces the BAM writers of tools/1.convert_AG_to_CT.py and tools/2.extend_gap.py and
 * fgbio SortBam -s TemplateCoordinate behind the rules convert_Bstrain, extend and
 * groupsort_convert, main.snake.py:121-153: the file fgbio CallDuplexConsensusReads reads at :163;
 * csrc/bsdc_toolrec.hip, DESIGN.md sections 3.10 and 8.11).  `out` is the bsdc_consensus of a
 * bsdc_run(.. | BSDC_MODE_DUMP) (dump_pos, dump_len, dump_tags, dump_seq, dump_qual; the last two
 * n_dump bytes each, 4-byte aligned) and rec the batch's record table (bsdc_family_batch.rec:
 * rec[4 r] = record r's offset in dump_seq / dump_qual).  tab: one bsdc_toolrec_rec per batch
 * record, the fields the tools leave as they are; names, cigar, aux: what its offsets point
 * into -- the read names (no NUL), the cigar ops with the leading and trailing S op removed, the
 * aux bytes (of a record tool 1 converts: with any RD / LA tag cut out).  Output record r is batch
 * record r: off [n_rec + 1] receives the exclusive prefix sum of the records' byte counts (off[n_rec]
 * = the total) and dst + off[r] the record: block_size; refID, pos = dump_pos, l_read_name, mapq,
 * bin = reg2bin(pos, pos + max(the new cigar's reference length, 1)), n_cigar_op, flag, l_seq =
 * dump_len, next_refID, next_pos, tlen; name NUL; the new cigar (tags bit1: 1M in front and, with
 * bit0, the last op one shorter or gone at length 1; else bit2: 1M in front; bit3: 1M behind; ops
 * never merged); the dump's nt16 codes two per byte, the pad nibble of an odd length 0; the dump's
 * quals; the aux bytes; with bit1, RD:C:bit0 and LA:C:1.  No byte at or past dst + cap is written.
 * bsdc_toolrec_bytes_bound = a size known before the launch, < 0 on a negative argument; tmp:
 * bsdc_toolrec_tmp_bytes of 8-byte aligned scratch.  bsdc_toolrec_format: device pointers but for
 * `out` itself and tab_host, the caller's host copy of tab, which is what gets checked; sizes,
 * scan and records are enqueued on `stream` (hipStream_t) by the one call, after the bsdc_run on
 * it.  bsdc_toolrec_host: host pointers, the same per-record functions run sequentially on the CPU
 * (no GPU needed) -- the twin the tests compare the kernel with, and the whole-file path's encoder.
 * BSDC_EINVAL, before anything is enqueued, with the reason in bsdc_toolrec_last_error (thread-
 * local): a NULL pointer (the dump buffers included), a negative count, a cap below the bound, a
 * misaligned buffer, a table entry that leaves names / cigar / aux, a name outside 1..254 bytes,
 * more than 65533 ops, more than 2^24 aux bytes; bsdc_toolrec_host also: a record whose dump slot
 * (rec[4 r] + dump_len[r]) leaves n_dump.  The launcher cannot read rec[] and dump_len, which lie
 * in HBM: there the kernel gives such a record l_seq 0 and reads nothing outside the dump, so the
 * caller passes the n_dump its dump buffers really hold. */
typedef struct {
    int64_t name_off;    /* first byte of the read name in names */
    int64_t cig_off;     /* first op in cigar */
    int64_t aux_off;     /* first aux byte in aux */
    int32_t aux_len;
    int32_t n_cig;       /* ops, clips removed */
    int32_t ref_id, next_ref_id, next_pos, tlen;
    uint16_t flag;
    uint8_t mapq;
    uint8_t name_len;    /* without the NUL */
    int32_t reserved;
} bsdc_toolrec_rec;

int64_t bsdc_toolrec_bytes_bound(int64_t n_rec, int64_t name_bytes, int64_t n_ops, int64_t aux_bytes, int64_t n_dump);
int64_t bsdc_toolrec_tmp_bytes(int64_t n_rec);
int32_t bsdc_toolrec_format(const bsdc_consensus *out, const uint32_t *rec, int64_t n_rec, int64_t n_dump,
                            const bsdc_toolrec_rec *tab, const bsdc_toolrec_rec *tab_host, const uint8_t *names,
                            int64_t name_bytes, const uint32_t *cigar, int64_t n_ops, const uint8_t *aux, int64_t aux_bytes,
                            int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream);
int32_t bsdc_toolrec_host(const bsdc_consensus *out, const uint32_t *rec, int64_t n_rec, int64_t n_dump,
                          const bsdc_toolrec_rec *tab, const uint8_t *names, int64_t name_bytes, const uint32_t *cigar,
                          int64_t n_ops, const uint8_t *aux, int64_t aux_bytes, int64_t *off, uint8_t *dst, int64_t cap);
const char *bsdc_toolrec_last_error(void);

/* (new exports, ABI 19 still) cli zipper: the aligned consensus records with their unmapped
 * partners' tags put back, in coordinate order (replaces `samtools sort -n | fgbio ZipperBams
 * --sort Coordinate | samtools view -F 4`, rules mergeAunA_consensus and
 * mergeAunA_consensus_grepaligned, main.snake.py:97-119; csrc/bsdc_zipper.hip, DESIGN.md sections
 * 3.11 and 8.12).
 *
 * bsdc_zip_sort: keys [n] (refID << 32 | (pos + 1) << 1 | reverse) and their payload idx [n], device
 * pointers, sorted in place by ascending key, equal keys in their order (a stable LSD radix sort,
 * 8 bits a pass); max_ref >= every refID and max_pos >= every pos of the keys: a pass whose digit
 * is zero in every key of that range is skipped.  tmp: bsdc_zip_sort_tmp_bytes(n) of 8-byte aligned
 * scratch.  Everything is enqueued on `stream`.  bsdc_zip_sort_host: the same on host pointers.
 * bsdc_zip_sort_tile: the keys a workgroup handles in a pass.
 *
 * bsdc_zip_format: output record k is table entry idx[k]: off [n + 1] receives the exclusive prefix
 * sum of the records' byte counts and dst + off[k] the record -- the aligned record's bytes up to
 * its aux (rec + rec_off, aux_start of them) with block_size the output's and flag bit 0x200
 * replaced by flag_or's; then its aux tags but those whose name the partner's aux (part +
 * part_off, part_len bytes) also holds and those named in tags->remove; then the partner's tags
 * but those in tags->remove, and, where the record's flag has 0x10: a Z or B tag named in
 * tags->reverse with its bytes / elements in reverse order, a Z tag named in tags->revcomp
 * reversed with A<->T, C<->G in both cases.  Tags are found by walking the aux by type.  No byte
 * at or past dst + cap is written; bsdc_zip_bytes_bound (of the host table) is a cap that holds.
 * idx, tab, rec, part, off, dst, tmp (bsdc_zip_format_tmp_bytes(n), 8-byte aligned): device
 * pointers; tab_host, rec_host, part_host: the caller's host copies, which are what gets checked;
 * rec and part 4-byte aligned.  BSDC_EINVAL before anything is enqueued, with the reason in
 * bsdc_zip_last_error (thread-local): a NULL pointer, a negative count, a table entry that leaves
 * rec / part, a cap below the bound, more than BSDC_ZIP_MAX_TAGS names in a list, and a record one
 * of whose aux blocks holds a tag of an unknown type or one that runs past the block (the message
 * names the entry and its read).  bsdc_zip_format_host: host pointers, the same per-record
 * functions run sequentially on the CPU.
 *
 * bsdc_zip_scan_host: the records of `bytes` (BAM records back to back, as they lie behind the
 * header) listed into out [cap] -> their count (call with out NULL to count), < 0 on a record that
 * is truncated or whose lengths leave it.
 *
 * (new exports, ABI 19 still) cli zipper --stream true (DESIGN.md 3.11 "Streaming", 8.12):
 *
 * bsdc_zip_scan_prefix_host: bsdc_zip_scan_host for a piece of a file: the whole records at the
 * front of `bytes` are listed and *consumed receives their bytes; a record cut by the end of the
 * piece ends the list and is no error.  A record whose fixed fields are there and whose lengths
 * leave it is an error (< 0), cut or not.
 *
 * bsdc_zip_gather: output record k is source record order[k]: off [n + 1] receives the exclusive
 * prefix sum of src_len[order[k]] (the offset scan bsdc_zip_format uses) and dst + off[k] the bytes
 * src + src_off[order[k]] .. + src_len[order[k]], unchanged.  One wavefront per record; dst is
 * written in aligned dwords, each built from aligned source dwords by a funnel shift, heads and
 * tails byte-wise, at any alignment of the records on both sides.  No byte at or past dst + cap is
 * written; no byte outside src .. src + src_bytes is read.  order, src_off, src_len, src, off, dst,
 * tmp (bsdc_zip_gather_tmp_bytes(n), 8-byte aligned): device pointers, src and dst 4-byte aligned;
 * order_host, src_off_host, src_len_host: the caller's host copies, which are what gets checked.
 * BSDC_EINVAL before anything is enqueued, with the reason in bsdc_zip_last_error: a NULL pointer,
 * a negative count, an entry that leaves src, an order entry >= n, a cap below the sum of the
 * lengths.  bsdc_zip_gather_host: the same on host pointers (no host copies: it checks what it
 * reads). */
#define BSDC_ZIP_MAX_TAGS 32
typedef struct {
    int64_t rec_off;   /* the aligned record (its block_size field) in rec */
    int64_t part_off;  /* the partner's first aux byte in part */
    int32_t rec_len;   /* block_size + 4 */
    int32_t aux_start; /* the aligned record's first aux byte, from rec_off */
    int32_t part_len;  /* the partner's aux bytes */
    uint32_t flag_or;  /* 0x200 where the partner's flag has it, else 0 */
} bsdc_zip_rec;

typedef struct {
    uint8_t reverse[2 * BSDC_ZIP_MAX_TAGS], revcomp[2 * BSDC_ZIP_MAX_TAGS], remove[2 * BSDC_ZIP_MAX_TAGS]; /* two bytes a name */
    int32_t n_reverse, n_revcomp, n_remove, reserved;
} bsdc_zip_tags;

typedef struct {
    int64_t off;      /* the record (its block_size field) in the bytes */
    int32_t len;      /* block_size + 4 */
    int32_t aux;      /* its first aux byte, from off */
    int32_t ref_id, pos;
    uint16_t flag;
    uint8_t name_len; /* without the NUL; the name starts at off + 36 */
    uint8_t reserved0;
    int32_t reserved;
} bsdc_zip_src;

int32_t bsdc_zip_sort_tile(void);
int64_t bsdc_zip_sort_tmp_bytes(int64_t n);
int32_t bsdc_zip_sort(uint64_t *keys, uint32_t *idx, int64_t n, int32_t max_ref, int32_t max_pos, uint8_t *tmp, void *stream);
int32_t bsdc_zip_sort_host(uint64_t *keys, uint32_t *idx, int64_t n, int32_t max_ref, int32_t max_pos);
int64_t bsdc_zip_bytes_bound(const bsdc_zip_rec *tab_host, int64_t n);
int64_t bsdc_zip_format_tmp_bytes(int64_t n);
int32_t bsdc_zip_format(const uint32_t *idx, int64_t n, const bsdc_zip_rec *tab, const bsdc_zip_rec *tab_host,
                        const uint8_t *rec, const uint8_t *rec_host, int64_t rec_bytes, const uint8_t *part,
                        const uint8_t *part_host, int64_t part_bytes, const bsdc_zip_tags *tags, int64_t *off, uint8_t *dst,
                        int64_t cap, uint8_t *tmp, void *stream);
int32_t bsdc_zip_format_host(const uint32_t *idx, int64_t n, const bsdc_zip_rec *tab, const uint8_t *rec, int64_t rec_bytes,
                             const uint8_t *part, int64_t part_bytes, const bsdc_zip_tags *tags, int64_t *off, uint8_t *dst,
                             int64_t cap);
int64_t bsdc_zip_scan_host(const uint8_t *bytes, int64_t n_bytes, bsdc_zip_src *out, int64_t cap);
int64_t bsdc_zip_scan_prefix_host(const uint8_t *bytes, int64_t n_bytes, bsdc_zip_src *out, int64_t cap, int64_t *consumed);
int64_t bsdc_zip_gather_tmp_bytes(int64_t n);
int32_t bsdc_zip_gather(const uint32_t *order, const uint32_t *order_host, int64_t n, const int64_t *src_off,
                        const int64_t *src_off_host, const int32_t *src_len, const int32_t *src_len_host, const uint8_t *src,
                        int64_t src_bytes, int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream);
int32_t bsdc_zip_gather_host(const uint32_t *order, int64_t n, const int64_t *src_off, const int32_t *src_len, const uint8_t *src,
                             int64_t src_bytes, int64_t *off, uint8_t *dst, int64_t cap);
const char *bsdc_zip_last_error(void);

/* (new exports, ABI 19 still) cli group: paired-UMI molecule ids for the templates of a tagged BAM
 * -- fgbio GroupReadsByUmi -s Paired restated, parity unpinned (the input of rule
 * CallMolecularConsensusReads; csrc/bsdc_group.hip, DESIGN.md sections 3.12 and 8.13).
 *
 * bsdc_group_assign: n templates in read-name order.  k0 / k1 [n]: the packed position key of the
 * lower / higher end (refID << 32 | biased 5' position << 1 | reverse: any encoding whose integer
 * order is rule 2's); umi [n]: the canonical UMI, two bits a base, first half << 32 | second half;
 * strand [n]: 0 top, 1 bottom; kmax [3] (host): a bound of k0, k1 and umi each (their maximum, or
 * the OR of all values), by which sort passes over zero digits are skipped.  Position groups are
 * the runs of equal (k0, k1) in ascending order; inside one, the templates of one umi form a node,
 * the nodes are ordered by count descending, then umi ascending; walking them in that order an
 * unassigned node becomes a root and enters a FIFO, and for each node p taken from the FIFO every
 * still-unassigned node c with count(c) <= count(p) / 2 + 1 and hamming(umi(p), umi(c)) <= edits
 * (0..3; differing bases over both halves) joins the root's molecule and enters the FIFO, in node
 * order.  Molecule ids count from 0 over the groups in order, roots in their order.  Outputs:
 * mol [n] the template's id; ab [n] 0 (/A) when its strand is that of the root node's first
 * template (the lowest in name order), else 1 (/B); order [n] the templates by (id, ab, name
 * order); stats [4] (host): position groups, nodes, molecules, the most nodes of a group.
 * arena 0: a group of more than 64 nodes is walked in LDS when it has at most
 * bsdc_group_lds_nodes() nodes, 1: always in the scratch.  tmp: bsdc_group_tmp_bytes(n), 8-byte
 * aligned.  All but kmax and stats are device pointers; the call synchronises `stream` (it reads
 * three counts back) and returns with everything done but the last sort, which is enqueued.
 * bsdc_group_assign_host: the same on host pointers, group by group with the same join function.
 *
 * bsdc_group_format: output record 2k / 2k + 1 is R1 / R2 of template order[k] (tab [2n]: template
 * t's records at 2t, 2t + 1): the input record's bytes with every tag named `tag` (two letters,
 * NUL-terminated; the aux walked by type) left out, <tag>:Z:<mol>/<A|B> appended and block_size
 * adjusted.  off [2n + 1] receives the records' offsets, off[2n] their bytes; no byte at or past
 * dst + cap is written (bsdc_group_bytes_bound of the host table is a cap that holds).  BSDC_EINVAL
 * before anything is enqueued, with the reason in bsdc_group_last_error (thread-local): a null
 * pointer, a table entry that leaves rec, a malformed aux block (the read is named), a cap below
 * the bound.  `order` is a device array the launcher does not read: an entry >= n makes a record of
 * size 0 there (bsdc_group_format_host refuses it).  tmp: bsdc_group_format_tmp_bytes(n).
 * bsdc_group_format_host: host pointers, the same per-record function run sequentially.
 * Limits: bsdc_group_assign n <= 2^30 templates (bsdc_zip_sort's), bsdc_group_format n <= 2^29
 * (2n records). */
typedef struct bsdc_group_rec {
    int64_t off; /* the record (its block_size field) in rec */
    int32_t len; /* its bytes, block_size field included */
    int32_t aux; /* where its aux block starts */
} bsdc_group_rec;

int32_t bsdc_group_lds_nodes(void);
int64_t bsdc_group_tmp_bytes(int64_t n);
int32_t bsdc_group_assign(const uint64_t *k0, const uint64_t *k1, const uint64_t *umi, const uint8_t *strand, int64_t n,
                          int32_t edits, const uint64_t *kmax, int32_t arena, uint32_t *mol, uint8_t *ab, uint32_t *order,
                          int64_t *stats, uint8_t *tmp, void *stream);
int32_t bsdc_group_assign_host(const uint64_t *k0, const uint64_t *k1, const uint64_t *umi, const uint8_t *strand, int64_t n,
                               int32_t edits, const uint64_t *kmax, uint32_t *mol, uint8_t *ab, uint32_t *order, int64_t *stats);
int64_t bsdc_group_bytes_bound(const bsdc_group_rec *tab_host, int64_t n_rec);
int64_t bsdc_group_format_tmp_bytes(int64_t n);
int32_t bsdc_group_format(const uint32_t *order, const uint32_t *mol, const uint8_t *ab, int64_t n, const bsdc_group_rec *tab,
                          const bsdc_group_rec *tab_host, const uint8_t *rec, const uint8_t *rec_host, int64_t rec_bytes,
                          const char *tag, int64_t *off, uint8_t *dst, int64_t cap, uint8_t *tmp, void *stream);
int32_t bsdc_group_format_host(const uint32_t *order, const uint32_t *mol, const uint8_t *ab, int64_t n, const bsdc_group_rec *tab,
                               const uint8_t *rec, int64_t rec_bytes, const char *tag, int64_t *off, uint8_t *dst, int64_t cap);
const char *bsdc_group_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
