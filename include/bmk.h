/*
 * bmk.h -- C ABI of the MI355X read-backed phaser of het SNV calls ("bucket-map links", part of libbmf.so).
 *
 * With --vcf-phase the tools say which alleles of neighbouring het SNV calls of the genotype caller (bmg.h) lie on the same
 * copy of the chromosome: a record that shows a letter at two het sites LINKS them.  The pileup's counters (bmp.h), the
 * genotype cells (bmg.h) and the strand cells (bmb.h) are all per position; this is the one pass that looks at several
 * positions together, so it has a state of its own: a table of small link counters over the sorted list of het sites.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records, the five parameters and the calls:
 * it does not depend on the order of the records, on how they are cut over bmk_add calls, or on the grid.
 *   The record layout, PLACED, COUNTED RECORD (the flags, skip, the long-CIGAR placeholder, l_seq == 0, mapq < min_mapq), the
 *   walk and the clipping of a block to [0, ref_len[refID]) are those of bmp.h.
 *
 *   PARAMETERS, five u32 in this order: min_mapq and min_bq (as in bmg.h; the command line's are those of --vcf, 0 and 13),
 *   min_links (>= 1; --phase-min-links, 2), min_frac_ppm (500 001 .. 1 000 000; --phase-min-frac, 0.8) and reach (1 .. 8;
 *   --phase-reach, 4).
 *
 *   PHASE SITES.  The input is the calls of bmg_call, 24 u32 each (BMG_CALL_WORDS).  A call is a phase site if it has
 *   BMG_VARIANT and its two letters (words 4 and 5) differ; a 1/2 het is one.  Sites are numbered 0 .. H - 1 in the order
 *   given, which must be strictly ascending in (reference, position).  Allele 0 of a site is its call's first letter (word 4),
 *   allele 1 its second (word 5).
 *
 *   OBSERVATION.  A counted record observes allele a (0 or 1) at site i if it has a base of an M, = or X op inside its clipped
 *   block at the site's position, the quality byte of that base is 0xFF or at least min_bq, its 4-bit code is 1, 2, 4 or 8 and
 *   its letter is allele a of the site.  Anything else is no observation: a D, an N, a low quality, a third letter, a code that
 *   is no letter, a position the record does not reach.
 *
 *   LINKS.  For every counted record and every two sites i < j that it observes with j - i <= reach, the counter
 *   link[i][j - i - 1][2 a_i + a_j] gains 1.  The distance j - i is in site numbers, not bases; two sites one record observes
 *   are on one reference.  Counters are u32: more than 2^32 - 1 on one counter, or on the sum of two of one cell, is OUTSIDE
 *   THE RULE.  Each record counts on its own.
 *
 *   DECISIVE LINK, PARENT, FLIP.  For a cell (c00, c01, c10, c11): cis = c00 + c11, trans = c01 + c10, big the larger, small
 *   the other.  The link is decisive if big >= min_links and, in u64, big x 1 000 000 >= min_frac_ppm x (cis + trans); as
 *   min_frac_ppm is above one half, a tie is never decisive.  The parent of site j is j - d for the smallest d in 1 .. reach
 *   with j - d >= 0, site j - d on the same reference and link[j - d][d - 1] decisive; its flip is 0 if cis wins and 1 if trans
 *   wins.  A site without such a d is a ROOT.
 *
 *   PHASE.  root(j) is reached by following parents, hap(j) is the XOR of the flips on that path; a root has hap 0.  Haplotype
 *   1 carries allele hap(j) at site j, haplotype 2 the other.  A site is PHASED if its block -- the sites with its root -- has
 *   at least two sites.  Blocks may interleave: that is legal in a VCF and is not repaired.
 *   The output per site is BMK_OUT_WORDS = 8 u32, in site order: 0 the index of its call among the calls given; 1 root (a site
 *   number); 2 the root's 0-based position; 3 hap; 4 flags (bit 0 PHASED, bit 1 ROOT); 5 d of the parent link, 0 for a root;
 *   6 and 7 cis and trans of that link, 0 for a root.
 *
 * LEFT OUT, on purpose: links across the two mates of a pair (each record counts on its own); indel calls as phase sites; hom
 * sites; HP/PS tags on the BAM records (the file is already deflated when the calls are known); any likelihood or MEC
 * optimisation over a block; a phase quality; trios and several samples.
 *
 * A context is used as bmk_begin, any number of bmk_add, bmk_finish, then bmk_phase and bmk_links in any order; bmk_begin may
 * be called again at any time and starts over.  The state on the device is the sorted site slots (references back to back as
 * in bmn.h, 4 bytes a site), 16 bytes of site data and reach x 4 u32 counters per site: nothing per reference position.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMK_ERR_ARG, runs nothing and leaves the context usable
 * (after a refused bmk_add the records added before it are still there).
 *   bmk_begin: a null pointer where data is needed (calls may be null with n_calls == 0); n_ref == 0, a length of 0, more bases
 *   than bmp_begin takes; reach outside 1 .. 8; min_links == 0; min_frac_ppm outside 500 001 .. 1 000 000; a phase site whose
 *   reference is >= n_ref, whose position lies beyond its reference or with a letter above 3; phase sites that do not ascend;
 *   2^31 phase sites or more.  n_calls == 0 or H == 0 succeeds, and every later call then launches nothing.
 *   bmk_add: what bmp_add checks, in its order; the checks of the data need no context; no bmk_begin before it, or a
 *   bmk_finish since.  n_records == 0 succeeds.
 *   bmk_finish: no bmk_begin before it, or a bmk_finish since.
 *   bmk_phase, bmk_links: no bmk_begin (bmk_phase: no bmk_finish) before it; first + count beyond H; a null pointer with
 *   count > 0.
 *
 * Conventions as in bmb.h: plain C types, int status (the codes are BMS_*'s), message in bmk_last_error(), no CPU path.
 * bucket-map_amd/host/phase.h states the same rule in plain C++ and writes the text, tests/phase_rule.py in Python.
 */
#ifndef BMK_H
#define BMK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMK_OK = 0, BMK_ERR_ARG = 1, BMK_ERR_HIP = 2 };
enum { BMK_MIN_MAPQ = 0, BMK_MIN_BQ = 1, BMK_MIN_LINKS = 2, BMK_MIN_FRAC_PPM = 3, BMK_REACH = 4, BMK_N_PARAMS = 5 };
enum { BMK_CALL_WORDS = 24, BMK_OUT_WORDS = 8, BMK_N_STATS = 4, BMK_MAX_REACH = 8 };
enum { BMK_PHASED = 1, BMK_ROOT = 2 };
enum { BMK_W_CALL = 0, BMK_W_ROOT = 1, BMK_W_ROOT_POS = 2, BMK_W_HAP = 3, BMK_W_FLAGS = 4, BMK_W_D = 5, BMK_W_CIS = 6, BMK_W_TRANS = 7 };
enum { BMK_S_SITES = 0, BMK_S_PHASED = 1, BMK_S_BLOCKS = 2, BMK_S_OBSERVATIONS = 3 };

typedef struct bmk_ctx bmk_ctx;

const char *bmk_last_error(void);

int  bmk_create(int32_t device, bmk_ctx **out);
void bmk_destroy(bmk_ctx *ctx);

/* Selects the phase sites among the n_calls calls (BMK_CALL_WORDS u32 each, as bmg_call writes them, ascending), uploads them
 * and zeroes their H x reach x 4 counters; *out_n_sites (may be null) receives H.  params points to the BMK_N_PARAMS values. */
int  bmk_begin(bmk_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params, const uint32_t *calls, uint64_t n_calls,
               uint64_t *out_n_sites);

/* Adds the links of the counted records among the n_records records of in[0, n_bytes) to the counters. */
int  bmk_add(bmk_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* Parents, roots and haps from everything added; out_stats (may be null) receives BMK_N_STATS u64: H, phased sites, blocks of
 * at least two sites, observations counted. */
int  bmk_finish(bmk_ctx *ctx, uint64_t *out_stats);

/* The BMK_OUT_WORDS u32 of sites first .. first + count - 1, after bmk_finish. */
int  bmk_phase(bmk_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* The reach x 4 counters of sites first .. first + count - 1: out[(k reach + d - 1) 4 + 2 a_i + a_j] for site i = first + k
 * and site j = i + d.  Cells that point beyond H or into another reference are zero. */
int  bmk_links(bmk_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* Times in ms (HIP events on the context's stream): the kernels of every bmk_add since bmk_begin, summed, and the kernels of
 * the last bmk_finish. */
int  bmk_last_stats(bmk_ctx *ctx, float *ms_add, float *ms_finish);

#ifdef __cplusplus
}
#endif
#endif
