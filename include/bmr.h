/*
 * bmr.h -- C ABI of the MI355X reference-block pass ("bucket-map reference blocks", part of libbmf.so).
 *
 * With --gvcf the tools write, beside the variant calls of --vcf, what the reads say where NO variant is called: every base
 * of every reference lies under a variant line or inside a hom-ref block that carries a confidence, so "no variant here, and
 * 40 reads say so" can be told from "no read reached this base".  The genotype caller of bmg.h keeps four cells for every
 * position, not only at the sites; this is one pass over all of them, a segmentation into runs, and per-run minima and sums.
 *
 * THE RULE IS EXACT, in integers only, and a function of the cells of a bmg_ctx, the reference bases, the band bounds and
 * the excluded intervals: it does not depend on how the records were cut over bmg_add calls, or on the grid.
 *
 *   INPUTS
 *   - a bmg_ctx after bmg_begin and any number of bmg_add: its references, its min_mapq, min_bq, q_absent, q_cap (which made
 *     the cells) and its cells.  Its prior is NOT used.
 *   - one byte per reference base, as bmp_begin takes them: A C G T in either case give R = 0 .. 3, any other byte R = 4 (none).
 *   - bands: n_bands u32 (0 .. 16), strictly ascending, each in 1 .. 99.
 *   - exclude: n_exclude intervals of three u32 (reference, start, end exclusive), in any order; they may overlap or touch.
 *
 *   PER POSITION p WITH R <= 3: n[a], Q[a], M(a) = 100 Q[a] + 477 n[a], T(a) = 301 n[a] and the ten costs L(g) exactly as
 *   bmg.h defines them, WITHOUT the prior (L, not L'):
 *     dp(p) = min(n[A] + n[C] + n[G] + n[T], 2^32 - 1);
 *     h(p)  = the smallest L(g) over the nine genotypes other than RR;
 *     gq(p) = min(99, (h - L(RR)) / 100) if L(RR) <= h, otherwise 0.
 *   The prior is left out on purpose: a position no read covers must come out at gq = 0, not at the prior's 30.
 *
 *   BAND, STATE AND BLOCKS
 *   - band(p) is the number of bounds <= gq(p): 0 .. n_bands.
 *   - A position is IN a block if R <= 3 and no excluded interval holds it.  A position with R = 4 is NO_ALLELE; an excluded
 *     position is EXCLUDED, even if R = 4.
 *   - A BLOCK is a maximal run, inside one reference, of consecutive IN positions of equal band.  Blocks are listed in
 *     (reference, start) order.  A block never spans two references; a band change, an excluded position or an R = 4
 *     position ends it.
 *   A block is BMR_BLOCK_WORDS = 8 u32: 0 reference; 1 start; 2 end (exclusive); 3 band; 4 min_gq, the smallest gq in the
 *   block; 5 min_dp, the smallest dp in the block; 6, 7 sum_dp, a u64 sum of dp with the low word first (fewer than 2^32
 *   positions of less than 2^32 each: it cannot overflow).
 *
 *   PER-POSITION VIEW, for tests: BMR_CONF_WORDS = 2 u32 per position.  Word 0 holds gq in bits 0-7 and the band in bits
 *   8-15; bit 16 is IN, bit 17 EXCLUDED, bit 18 NO_ALLELE, exactly one of the three is set; gq and band are 0 unless IN.
 *   Word 1 holds dp, filled for every position.
 *
 *   By hand, at min_bq 13, q_cap 60 and all qualities 30: no base gives gq 0; 10 reference bases h = 3010 and gq 30; 40
 *   reference bases 99; 5 reference and 5 of one other letter 0 (RR loses); 9 reference and one other letter of quality 20
 *   L(RR) = 2477, h = 3010 and gq 5.
 *
 * LEFT OUT, on purpose: <NON_REF> likelihoods on the variant lines; PL in the blocks; a median DP; a maximal block length;
 * strand and position bias (bmb.h annotates the variant lines, not the blocks); several samples; windows for genomes whose state does not fit.
 *
 * bmr_run does not end the counting of the bmg_ctx and changes nothing in it: a bmg_add followed by a second bmr_run gives
 * the blocks of everything added by then, a bmg_begin followed by bmr_run starts from the new references, and it may be
 * called any number of times on one bmr_ctx.  bmr_blocks and bmr_conf_at return what the last successful bmr_run left; they
 * do not look at the bmg_ctx again.  On the device the module holds, beyond bmg's 32 bytes per base, 17 bytes per base (the
 * reference byte, the two words of the per-position view, a head flag and its rank, 4 bytes each) and 32 bytes per block, the
 * band bounds and 16 bytes per excluded interval.  What does not fit into free device memory is BMR_ERR_HIP with the sizes in
 * the message.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMR_ERR_ARG, runs nothing and leaves both contexts
 * usable (after a refused bmr_run the blocks of the run before it are still there).
 *   bmr_create: a null pointer.
 *   bmr_run: a null context, cells context, ref_bases or out_n_blocks; a null bands with n_bands > 0 or a null exclude with
 *   n_exclude > 0; no bmg_begin on the cells context; the two contexts on different devices; a null ref_bases entry;
 *   n_bands > 16, or a bound of 0, above 99, or not above its predecessor; an interval whose reference is >= n_ref, whose
 *   start >= end, or whose end lies beyond its reference.  n_exclude == 0 and n_bands == 0 succeed.
 *   bmr_blocks: a null context; no bmr_run before it; first + count beyond the number of blocks; a null pointer with count > 0.
 *   bmr_conf_at: a null context; no bmr_run before it; ref >= n_ref, start + count beyond the reference; a null pointer with
 *   count > 0.
 *   bmr_last_stats: a null context.
 *
 * Conventions as in bmg.h: plain C types, int status (the codes are BMS_*'s), message in bmr_last_error(), no CPU path.
 * bucket-map_amd/host/refblocks.h states the same rule in plain C++ and writes the gVCF, tests/refblocks_rule.py in Python.
 */
#ifndef BMR_H
#define BMR_H

#include <stdint.h>

#include "bmg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BMR_OK = 0, BMR_ERR_ARG = 1, BMR_ERR_HIP = 2 };
enum { BMR_MAX_BANDS = 16, BMR_BLOCK_WORDS = 8, BMR_CONF_WORDS = 2, BMR_EXCLUDE_WORDS = 3 };
enum { BMR_IN = 1 << 16, BMR_EXCLUDED = 1 << 17, BMR_NO_ALLELE = 1 << 18 };
enum { BMR_W_REF = 0, BMR_W_START = 1, BMR_W_END = 2, BMR_W_BAND = 3, BMR_W_MIN_GQ = 4, BMR_W_MIN_DP = 5, BMR_W_SUM_DP = 6 };

typedef struct bmr_ctx bmr_ctx;

const char *bmr_last_error(void);
int  bmr_create(int32_t device, bmr_ctx **out);
void bmr_destroy(bmr_ctx *ctx);

/* The blocks of everything added to cells so far.  ref_bases[r] points to the bases of reference r, as many as bmg_begin was
 * given for it.  *out_n_blocks receives the number of blocks. */
int  bmr_run(bmr_ctx *ctx, bmg_ctx *cells, const uint8_t *const *ref_bases, const uint32_t *bands, uint32_t n_bands, const uint32_t *exclude,
             uint64_t n_exclude, uint64_t *out_n_blocks);

/* Blocks first .. first + count - 1 of the last bmr_run: BMR_BLOCK_WORDS u32 each. */
int  bmr_blocks(bmr_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* The per-position view of positions start .. start + count - 1 of reference ref in the last bmr_run: BMR_CONF_WORDS u32 each. */
int  bmr_conf_at(bmr_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out);

/* The kernels of the last bmr_run in ms (HIP events on the context's stream; the uploads and the read of the block
 * count between them are not in it), and the bytes the module holds on the device. */
int  bmr_last_stats(bmr_ctx *ctx, float *ms_kernels, uint64_t *bytes_state);

#ifdef __cplusplus
}
#endif
#endif
