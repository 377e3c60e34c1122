/*
 * bmb.h -- C ABI of the MI355X strand-bias and mapping-quality annotator ("bucket-map bias", part of libbmf.so).
 *
 * With --vcf-bias the tools say, at every variant SNV call of the genotype caller (bmg.h), on which strand the counted bases
 * of each letter lay, how well their records were mapped (MQ) and how unlikely the split of the reference and the alternative
 * bases over the strands is (FS, the phred of Fisher's exact test).  The pileup's counters (bmp.h) and the genotype cells
 * (bmg.h) know neither the strand nor the MAPQ of a base, so this is a third pass of the shared walk with a state of its own.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records, the two parameters, the two tables
 * and the calls asked for: it does not depend on the order of the records, on how they are cut over bmb_add calls, on the
 * grid, or on how a sum is divided over lanes (every sum is of u64 and cannot wrap, see below).
 *   The record layout, PLACED, COUNTED RECORD (the flags, skip, the long-CIGAR placeholder, l_seq == 0, mapq < min_mapq), the
 *   walk and the clipping of a block to [0, ref_len[refID]) are those of bmp.h; WHICH BASES COUNT is bmg.h's: a base of an M, =
 *   or X op inside the clipped block whose quality byte is 0xFF or at least min_bq and whose 4-bit code is 1, 2, 4 or 8.
 *
 *   PARAMETERS, two u32 in this order: min_mapq and min_bq (as in bmp.h).  The command line's are those of --vcf: 0 and 13.
 *   Nothing else is needed: the caps of FS (6000) and of N (65 535) belong to the rule, the thresholds of the two filters to
 *   the writer of the file.
 *
 *   STATE, 40 bytes per reference position.
 *   - four u64 STRAND CELLS, one per letter A, C, G, T; a cell is fwd << 32 | rev.  A counted base of a record without the
 *     flag 0x10 adds 1 << 32 to its letter's cell at its position, one of a record with 0x10 adds 1.  With equal min_mapq and
 *     min_bq, fwd + rev of letter a is bmg.h's n[a] at every position.
 *   - one u64 MAPQ CELL, n << 40 | S.  Every counted base adds (1 << 40) + mapq^2, mapq the byte 13 of its record.
 *   More than 2^24 - 1 counted bases on one position are OUTSIDE THE RULE; up to there S <= 65 025 x 16 777 215 < 2^40 cannot
 *   carry into n.
 *
 *   PER CALL.  The input is a call of bmg_call, 24 u32 (BMG_CALL_WORDS).  Only a call with BMG_VARIANT is annotated; the
 *   annotation of any other is sixteen zeros.  With fwd[a], rev[a], n, S of the five cells at (reference, position), R the
 *   call's reference allele and g* its two letters:
 *   - MQ = isqrt(10000 S / n) (the division floors first), the floor of the root mean square of the MAPQs in centi-units;
 *     0 where n == 0.  10000 S < 2^54.
 *   - THE TABLE: a = fwd[R], b = rev[R]; c and d are fwd and rev summed over the distinct letters of g* other than R.  Rows
 *     are the reference and the alternative, columns the strands.  r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d.
 *   - FS, in centi-phred, from two tables of integers that are INPUTS of the rule:
 *       LF[n] = round(1000 log10(n!)), n = 0 .. 65 535, u32;     E[k] = round(2^40 10^(-k / 1000)), k = 0 .. 12 000, u64.
 *     bmb_tables makes both on the host, in long double; a context uploads what bmb_tables gives.  host/bias.h and
 *     tests/bias_rule.py take the tables as arguments and never compute them, so all three agree whatever the last bit of a
 *     libm is.
 *       x runs over max(0, c1 - r2) .. min(r1, c1);   w(x) = -(LF[x] + LF[r1 - x] + LF[c1 - x] + LF[r2 - c1 + x]);
 *       m = the largest w(x);   S_all = the sum of E[m - w(x)] over all x, E taken as 0 beyond its end;
 *       S_ext = the same sum over the x with w(x) <= w(a) + 4;
 *       FS = min(6000, the smallest k with S_all E[k] <= S_ext 2^40), a 128-bit compare of two products.
 *     The 4 is the rounding of four table entries on either side: tables of equal probability tie, as the relative
 *     tolerance of R's fisher.test makes them.  At most 65 536 terms of at most 2^40: the sums are below 2^57.
 *     A table with a + b + c + d > 65 535 or with a zero margin (r1, r2, c1 or c2) has NO FS: the flag BMB_NO_FS and FS 0.
 *   An annotation is BMB_OUT_WORDS = 16 u32: 0 .. 3 fwd[A .. T]; 4 .. 7 rev[A .. T]; 8 MQ; 9 FS; 10 flags (bit 0 ANNOTATED,
 *   bit 1 NO_FS); 11 n; 12 .. 15 a, b, c, d.
 *
 * LEFT OUT, on purpose: capping a base's quality by its record's MAPQ inside the genotype rule (the calls do not change);
 * SOR; read-position and base-quality rank tests; MQ0; annotations on indel lines and in the <NON_REF> blocks; several
 * samples; a cheaper difference-array form of the mapq cell (a record's MAPQ is the same at all its positions).
 *
 * A context is used as bmb_begin, then any number of bmb_add, bmb_annotate and bmb_cells_at in any order; bmb_begin may be
 * called again at any time and starts over.  The state on the device is a [position][4] u64 array of strand cells, 32 bytes
 * = one sector per position, and a [position] u64 array of mapq cells, over the references back to back; beside bmp's 33 and
 * bmg's 32 bytes that is 105 per base.  The two tables (262 144 + 96 008 bytes) are uploaded by bmb_create.  What does not
 * fit into free device memory is BMB_ERR_HIP with the sizes in the message.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMB_ERR_ARG, runs nothing and leaves the context
 * usable (after a refused bmb_add the records added before it are still there).
 *   bmb_begin: n_ref == 0, a length of 0, more bases than bmp_begin takes, a null pointer.
 *   bmb_add: what bmp_add checks, in its order; the checks of the data need no context.  n_records == 0 succeeds.
 *   bmb_annotate: a null pointer with n_calls > 0; 2^31 calls or more; no bmb_begin before it; a VARIANT call whose reference
 *   is >= n_ref, whose position lies beyond its reference, or whose R or letters are above 3.  n_calls == 0 succeeds and
 *   launches nothing.
 *   bmb_cells_at: no bmb_begin before it; ref >= n_ref, start + count beyond the reference; both pointers null with count > 0.
 *
 * Conventions as in bmg.h: plain C types, int status (the codes are BMS_*'s), message in bmb_last_error(), no CPU path.
 * bucket-map_amd/host/bias.h states the same rule in plain C++ and writes the text, tests/bias_rule.py in Python.
 */
#ifndef BMB_H
#define BMB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMB_OK = 0, BMB_ERR_ARG = 1, BMB_ERR_HIP = 2 };
enum { BMB_MIN_MAPQ = 0, BMB_MIN_BQ = 1, BMB_N_PARAMS = 2 };
enum { BMB_N_STRAND_CELLS = 4, BMB_CALL_WORDS = 24, BMB_OUT_WORDS = 16 };
enum { BMB_N_LF = 65536, BMB_N_E = 12001, BMB_FS_CAP = 6000, BMB_FS_MAX_N = 65535 };
enum { BMB_ANNOTATED = 1, BMB_NO_FS = 2 };
enum { BMB_W_FWD = 0, BMB_W_REV = 4, BMB_W_MQ = 8, BMB_W_FS = 9, BMB_W_FLAGS = 10, BMB_W_N = 11, BMB_W_TABLE = 12 };

typedef struct bmb_ctx bmb_ctx;

const char *bmb_last_error(void);

/* The two tables of the FS rule, computed in long double on the host: lf[0 .. BMB_N_LF), e[0 .. BMB_N_E).  Needs no device. */
int  bmb_tables(uint32_t *lf, uint64_t *e);

int  bmb_create(int32_t device, bmb_ctx **out);
void bmb_destroy(bmb_ctx *ctx);

/* Sizes the state for the n_ref references and zeroes the cells.  params points to the BMB_N_PARAMS values in the order above. */
int  bmb_begin(bmb_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params);

/* Adds the counted records among the n_records records of in[0, n_bytes) to the cells. */
int  bmb_add(bmb_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* The annotations of the n_calls calls (BMB_CALL_WORDS u32 each, as bmg_call writes them, in any order) from everything added
 * so far: BMB_OUT_WORDS u32 each, in the order of the calls. */
int  bmb_annotate(bmb_ctx *ctx, const uint32_t *calls, uint64_t n_calls, uint32_t *out);

/* The cells of positions start .. start + count - 1 of reference ref: strand[4 * k .. 4 * k + 3] and mapq[k]; either may be null. */
int  bmb_cells_at(bmb_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint64_t *strand, uint64_t *mapq);

/* Times in ms (HIP events on the context's stream): the kernels of every bmb_add since bmb_begin, summed, and the kernel of
 * the last bmb_annotate. */
int  bmb_last_stats(bmb_ctx *ctx, float *ms_add, float *ms_annotate);

#ifdef __cplusplus
}
#endif
#endif
