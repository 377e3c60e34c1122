/*
 * bmg.h -- C ABI of the MI355X genotype caller ("bucket-map genotypes", part of libbmf.so).
 *
 * With --vcf the tools call, at every SNV site of the pileup (bmp.h), the diploid genotype of the sample from the base
 * qualities of the records they have just written, and write a VCF.  The pileup's counters keep how many reads show a letter,
 * not how good those bases were, so this is a second pass over the records with a state of its own; the records are still at
 * hand when the file is done (the sorter of bms.h holds them).
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records, the five parameters and the sites
 * asked for: it does not depend on the order of the records, on how they are cut over bmg_add calls, or on the grid.
 *   The record layout, PLACED, COUNTED RECORD (the flags, skip, the long-CIGAR placeholder, l_seq == 0, mapq < min_mapq), the
 *   walk and the clipping of a block to [0, ref_len[refID]) are those of bmp.h and are not repeated here.
 *
 *   PARAMETERS, five u32 in this order: min_mapq and min_bq (as in bmp.h); q_absent, the quality a base with the quality byte
 *   0xFF is given; q_cap, the most a base quality counts for (1 .. 93, and q_absent <= q_cap); prior, in centi-phred, the cost
 *   of each distinct non-reference allele in a genotype.  The command line's are 0, 13, 30, 60, 3000.
 *
 *   FOUR u64 CELLS PER REFERENCE POSITION, one per letter A, C, G, T; a cell is n << 32 | Q, the number of bases and the sum
 *   of their qualities.
 *   - A base of an M, = or X op inside the clipped block of a counted record, with the quality byte q and the 4-bit code of
 *     the sequence as in bmp.h, adds to a cell only if q == 0xFF or q >= min_bq, and the code is 1, 2, 4 or 8 (A, C, G, T).  It
 *     adds (1 << 32) + q_eff to its letter's cell at its position, q_eff = q == 0xFF ? q_absent : min(q, q_cap).
 *   - Nothing else adds anything: not a base of low quality or of another code, not D, I, N, S, H or P.
 *   More than floor((2^32 - 1) / q_cap) counted bases of one letter at one position are OUTSIDE THE RULE: beyond that the
 *   low word may carry into the count (at q_cap 60 that is 71 582 788 bases on one position).
 *   With equal min_mapq and min_bq, n of letter a is bmp.h's counter a at every position.
 *
 *   CALLS.  A site is twelve u32 as bmp_sites returns it: reference, position, R = the reference allele (0 .. 3, or 4 for
 *   none), the eight counters (not looked at), the kind bits.  With n[a], Q[a] of the four cells at (reference, position):
 *   - a base of the error probability e = 10^(-q/10) that shows letter c costs, in -10 log10 of its probability, about q +
 *     4.77 under a genotype without c (e / 3), 3.01 under a heterozygous one with c ((1 - e) / 2 + e / 6, taken as 1 / 2) and
 *     0 under cc (1 - e, taken as 1: the term 1 - e is dropped on purpose).  In centi-phred and u64, per letter:
 *       M(a) = 100 Q[a] + 477 n[a],   T(a) = 301 n[a]
 *   - the ten genotypes {a <= b} have the index k = b (b + 1) / 2 + a: AA AC CC AG CG GG AT CT GT TT;
 *       L(aa) = the sum of M(c) over c != a,   L(ab) = T(a) + T(b) + the sum of M(c) over c not in {a, b},
 *       L'(g) = L(g) + prior x (the number of distinct letters of g other than R);
 *   - g* has the smallest L'; a tie goes to RR if RR is among the tied, otherwise to the smallest k;
 *   - GQ = min(99, (the second smallest L' of the ten, as a multiset -- equal to the smallest on a tie -- minus L'(g*)) / 100);
 *   - qual = min(L'(RR) - L'(g*), 2^32 - 1);  PL[k] = min(L'(k) - L'(g*), 2^32 - 1);  DP = min(n[A] + n[C] + n[G] + n[T], 2^32 - 1).
 *   A call is BMG_CALL_WORDS = 24 u32: 0 .. 2 reference, position, R; 3 flags (bit 0 GENOTYPED, bit 1 VARIANT: g* != RR);
 *   4 .. 5 the letters of g*, the smaller first; 6 GQ; 7 qual; 8 .. 11 n[A .. T]; 12 .. 21 PL[0 .. 9]; 22 DP; 23 zero.
 *   A site without the SNV kind bit, with R above 3, or with DP == 0 is not genotyped: flags 0 and zeros in 4 .. 7 and
 *   12 .. 23; its words 0 .. 2 and its n are filled all the same.
 *
 * LEFT OUT, on purpose: indel alleles and calls; capping a base's quality by its record's MAPQ; removing the overlap of two
 * mates (a fragment's overlap counts twice, unless the records were written with `--clip-overlap`); a ploidy other than 2; several samples; strand or position bias in the calls (bmb.h annotates the strands and the MAPQ beside them); windows for
 * genomes whose state does not fit.
 *
 * A context is used as bmg_begin, then any number of bmg_add, bmg_call and bmg_cells_at in any order: bmg_call does not end
 * the counting, a bmg_add after it keeps counting.  bmg_begin may be called again at any time and starts over.  No reference
 * bases are needed: the sites carry R.  The state on the device is [position][4] u64 over the references back to back, 32
 * bytes = one sector per position; beside the pileup's 33 that is 65 bytes per base, about 202 GB at 3.1 Gbp.  The sites of
 * a bmg_call are uploaded per call into a buffer of the context, 48 bytes in and 96 bytes out per site.  What does not fit
 * into free device memory is BMG_ERR_HIP with the sizes in the message.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMG_ERR_ARG, runs nothing and leaves the context
 * usable (after a refused bmg_add the records added before it are still there).
 *   bmg_begin: n_ref == 0, a length of 0, more bases than bmp_begin takes, q_cap == 0, q_cap > 93, q_absent > q_cap, a null
 *   pointer.
 *   bmg_add: what bmp_add checks, in its order; the checks of the data need no context.  n_records == 0 succeeds.
 *   bmg_call: a null pointer with n_sites > 0; no bmg_begin before it; a site whose reference is >= n_ref or whose position
 *   lies beyond its reference.  n_sites == 0 succeeds.
 *   bmg_cells_at: no bmg_begin before it; ref >= n_ref, start + count beyond the reference; a null pointer with count > 0.
 *
 * Conventions as in bmp.h: plain C types, int status (the codes are BMS_*'s), message in bmg_last_error(), no CPU path.
 * bucket-map_amd/host/genotype.h states the same rule in plain C++ and writes the VCF, tests/genotype_rule.py in Python.
 */
#ifndef BMG_H
#define BMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMG_OK = 0, BMG_ERR_ARG = 1, BMG_ERR_HIP = 2 };
enum { BMG_MIN_MAPQ = 0, BMG_MIN_BQ = 1, BMG_Q_ABSENT = 2, BMG_Q_CAP = 3, BMG_PRIOR = 4, BMG_N_PARAMS = 5 };
enum { BMG_N_CELLS = 4, BMG_N_GENOTYPES = 10, BMG_SITE_WORDS = 12, BMG_CALL_WORDS = 24 };
enum { BMG_GENOTYPED = 1, BMG_VARIANT = 2 };
enum { BMG_W_REF = 0, BMG_W_POS = 1, BMG_W_R = 2, BMG_W_FLAGS = 3, BMG_W_GT = 4, BMG_W_GQ = 6, BMG_W_QUAL = 7, BMG_W_N = 8, BMG_W_PL = 12, BMG_W_DP = 22 };

typedef struct bmg_ctx bmg_ctx;

const char *bmg_last_error(void);
int  bmg_create(int32_t device, bmg_ctx **out);
void bmg_destroy(bmg_ctx *ctx);

/* Sizes the state for the n_ref references and zeroes the cells.  params points to the BMG_N_PARAMS values in the order above. */
int  bmg_begin(bmg_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params);

/* Adds the counted records among the n_records records of in[0, n_bytes) to the cells. */
int  bmg_add(bmg_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* The calls of the n_sites sites (BMG_SITE_WORDS u32 each, in any order) from everything added so far: BMG_CALL_WORDS u32
 * each, in the order of the sites. */
int  bmg_call(bmg_ctx *ctx, const uint32_t *sites, uint64_t n_sites, uint32_t *out);

/* The BMG_N_CELLS cells of positions start .. start + count - 1 of reference ref: out[4 * k .. 4 * k + 3]. */
int  bmg_cells_at(bmg_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint64_t *out);

/* Times in ms (HIP events on the context's stream): the kernels of every bmg_add since bmg_begin, summed, and the kernel of
 * the last bmg_call. */
int  bmg_last_stats(bmg_ctx *ctx, float *ms_add, float *ms_call);

#ifdef __cplusplus
}
#endif
#endif
