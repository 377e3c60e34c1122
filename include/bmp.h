/*
 * bmp.h -- C ABI of the MI355X pileup counter ("bucket-map pileup", part of libbmf.so).
 *
 * With --pileup the tools report, for the BAM records they have just written, what the reads say at every base of every
 * reference -- how many show A, C, G, T, another letter, a deletion, an insertion behind it, or a base of low quality -- and
 * list the positions where enough of them disagree with the reference.  The records are still at hand when the file is done
 * (the sorter of bms.h holds them) and the genome is in host memory, so no second program has to read and inflate the file
 * and walk every CIGAR again.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records, the references and the four
 * thresholds: it does not depend on the order of the records, on how they are cut over bmp_add calls, or on the grid.
 *   The record layout, PLACED, the long-CIGAR placeholder and the walk are those of bmc.h and are not repeated here: the ops
 *   of a record are walked with a reference cursor that starts at pos and a query cursor that starts at 0 (both 64-bit); M, =
 *   and X advance both and form a block, D and N advance the reference cursor only, I and S the query cursor only, H and P
 *   neither; a block is clipped to [0, ref_len[refID]), and what lies beyond the end of the reference is not counted, and its
 *   query bases are not either.
 *
 *   THRESHOLDS, four u32 in this order: min_mapq, min_bq, min_alt (at least 1), min_frac_ppm (0 .. 1 000 000).
 *
 *   COUNTED RECORD.  A placed record is counted unless
 *   - its CIGAR is the long-CIGAR placeholder, or its l_seq is 0: it adds 1 to n_left_out of its reference, nothing else;
 *   - its mapq < min_mapq: it adds 1 to n_low_mapq of its reference, nothing else.
 *   A record of which both hold goes to n_left_out.
 *
 *   EIGHT u32 COUNTERS PER REFERENCE POSITION, in the order A, C, G, T, N, DEL, INS, LOWQ.
 *   - Every base of an M, = or X op inside the clipped block has a query index j and the quality q = qual[j].  If q != 0xFF
 *     and q < min_bq, LOWQ += 1 at its position.  Otherwise the 4-bit code of the sequence (byte j / 2, the high nibble for
 *     even j) selects the counter: 1 -> A, 2 -> C, 4 -> G, 8 -> T, every other code -> N.  A quality of 0xFF (absent) always
 *     passes.
 *   - D: DEL += 1 at every position of the op that lies inside the reference.  N, S, H and P add nothing.
 *   - I (of a length > 0): INS += 1 at the anchor, the reference cursor - 1.  It counts only if an M, =, X or D op with a
 *     length > 0 precedes it in the record and the anchor lies inside the reference: a leading insertion is dropped (also one
 *     straight after S, H, P or N), and so is one that hangs off the end of the reference.
 *   span(p) = A + C + G + T + N + DEL.
 *
 *   REFERENCE BASES.  One byte per base.  A C G T in either case give the reference allele 0 .. 3; any other byte gives none
 *   (4).
 *
 *   SITES.  Position p is a site of the kinds SNV, DEL, INS (bits 1, 2, 4):
 *   - SNV: p has a reference allele, and the largest count `alt` among the other three of A, C, G, T has alt >= min_alt and
 *     alt * 1 000 000 >= min_frac_ppm * span(p), in u64;
 *   - DEL: the same two tests on the DEL counter;  INS: the same two tests on the INS counter (against the same span(p)).
 *   A position is listed once, with the OR of its kinds, in (reference, position) order.  A site is twelve u32: reference,
 *   position, reference allele (0 .. 3, or 4 for none), the eight counters, the kind bits.
 *
 *   PER REFERENCE, six u64: n_reads (the counted records on it), n_low_mapq, n_left_out, n_bases (the sum of A .. N over
 *   its positions), n_lowq (the sum of LOWQ), n_sites.
 *
 * LEFT OUT, on purpose: the alleles, lengths and sequences of indels (only that there is one); the CG:B,I tag of a record
 * with the placeholder (KNOWN DEPARTURE, as in bmc.h: such a record is left out and counted in n_left_out); removing the
 * overlap of two mates (a fragment's overlap counts twice, unless the records were written with `--clip-overlap`); genotypes and their likelihoods; VCF; windows for genomes whose
 * state does not fit.
 *
 * A context is used as bmp_begin, any number of bmp_add, bmp_finish, then any number of bmp_sites / bmp_counts_at; bmp_begin
 * may be called again at any time and starts over (nothing of the earlier references, thresholds or records remains).  The
 * state on the device is counter-major, [position][8] u32 over the references back to back, and one byte of reference per
 * position: 33 bytes per base (32 of counters, one sector per position, and 1 of reference; 103 GB at 3.1 Gbp), and 48 bytes
 * per listed site.  What does not fit into free device memory is BMP_ERR_HIP with the sizes in the message.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMP_ERR_ARG, runs nothing and leaves the context
 * usable (after a refused bmp_add the records added before it are still there).
 *   bmp_begin: n_ref == 0, a length of 0, more than 2^32 - 2^20 bases in all (or 2^32 - 1 or more with one more per
 *   reference: bmc_begin's limit), min_alt == 0, min_frac_ppm > 1 000 000, a null pointer, a null ref_bases entry.
 *   bmp_add: what bmc_add checks, in its order -- the stream (bms.h, and the fields of every record lie inside it); an op
 *   code above 8; n_cigar_op > 0, l_seq != 0 and the summed M, I, S, =, X lengths differ from l_seq; a null pointer (skip may
 *   be null); these need no context.  Then, with the context: no bmp_begin before it, or a bmp_finish since; refID >= n_ref
 *   on a record without flag 0x4.  n_records == 0 succeeds.
 *   bmp_finish: no bmp_begin before it, or a second bmp_finish; a null pointer.
 *   bmp_sites / bmp_counts_at: no bmp_finish before it; first + count beyond the sites, ref >= n_ref, start + count beyond
 *   the reference; a null pointer with count > 0.
 * The context is looked at last, so the checks of the data need no device.
 *
 * Conventions as in bms.h: plain C types, int status, message in bmp_last_error(), no CPU path.
 * bucket-map_amd/host/pileup.h states the same rule in plain C++, tests/pileup_rule.py in Python.
 */
#ifndef BMP_H
#define BMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMP_OK = 0, BMP_ERR_ARG = 1, BMP_ERR_HIP = 2 };
enum { BMP_A = 0, BMP_C = 1, BMP_G = 2, BMP_T = 3, BMP_N = 4, BMP_DEL = 5, BMP_INS = 6, BMP_LOWQ = 7, BMP_N_COUNTERS = 8 };
enum { BMP_MIN_MAPQ = 0, BMP_MIN_BQ = 1, BMP_MIN_ALT = 2, BMP_MIN_FRAC_PPM = 3, BMP_N_THRESHOLDS = 4 };
enum { BMP_KIND_SNV = 1, BMP_KIND_DEL = 2, BMP_KIND_INS = 4, BMP_SITE_WORDS = 12 };
enum { BMP_N_READS = 0, BMP_N_LOW_MAPQ = 1, BMP_N_LEFT_OUT = 2, BMP_N_BASES = 3, BMP_N_LOWQ = 4, BMP_N_SITES = 5, BMP_N_STATS = 6 };

typedef struct bmp_ctx bmp_ctx;

const char *bmp_last_error(void);
int  bmp_create(int32_t device, bmp_ctx **out);
void bmp_destroy(bmp_ctx *ctx);

/* Sizes the state for the n_ref references, zeroes the counters and uploads the reference bases: ref_bases[r] points to
 * ref_len[r] bytes.  thresholds points to the BMP_N_THRESHOLDS values in the order above. */
int  bmp_begin(bmp_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref, const uint8_t *const *ref_bases, const uint32_t *thresholds);

/* Adds the counted records among the n_records records of in[0, n_bytes) to the counters. */
int  bmp_add(bmp_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* The sites and sums of everything added: *out_n_sites, and out_ref_stats[BMP_N_STATS * r + k] in the order above. */
int  bmp_finish(bmp_ctx *ctx, uint64_t *out_n_sites, uint64_t *out_ref_stats);

/* Sites first .. first + count - 1, BMP_SITE_WORDS u32 each. */
int  bmp_sites(bmp_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* The BMP_N_COUNTERS counters of positions start .. start + count - 1 of reference ref: out[8 * k .. 8 * k + 7]. */
int  bmp_counts_at(bmp_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out);

/* Times in ms (HIP events on the context's stream): the kernels of every bmp_add since bmp_begin, summed, and bmp_finish's
 * passes and scan (it includes the host's read of the site count). */
int  bmp_last_stats(bmp_ctx *ctx, float *ms_add, float *ms_finish);

#ifdef __cplusplus
}
#endif
#endif
