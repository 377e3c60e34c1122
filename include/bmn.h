/*
 * bmn.h -- C ABI of the MI355X indel caller ("bucket-map indels", part of libbmf.so).
 *
 * With --vcf-indels the tools add to the VCF of bmg.h the insertions and deletions the records they have just written carry:
 * WHICH indel a read shows at an anchor (bmp.h only counts THAT it shows one), the table of the distinct ones with their
 * counts, and a diploid call per anchor.  It is a pass over the CIGARs only: no base qualities are read, and sequence bytes
 * only under an insertion.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records and the five parameters: it does not
 * depend on the order of the records, on how they are cut over bmn_add calls, or on the grid.
 *   The record layout, PLACED, COUNTED RECORD (the flags 0x4 | 0x100 | 0x200 | 0x400, skip, the long-CIGAR placeholder and
 *   l_seq == 0 to n_left_out, mapq < min_mapq to n_low_mapq) and the cursors of the walk are those of bmp.h and bmc.h and are
 *   not repeated here.  Per reference, three u64: n_reads (the counted records on it), n_low_mapq, n_left_out; for an equal
 *   min_mapq they are bmp.h's.
 *
 *   PARAMETERS, five u32 in this order: min_mapq; min_alt (at least 1); min_frac_ppm (0 .. 1 000 000); q_indel, the phred
 *   quality every indel observation is given (1 .. 93); prior, in centi-phred, the cost of a genotype with the ALT in it.
 *   The command line's are 0, 2, 200 000, 30, 4000.
 *
 *   EXTENT AND COVER.  end is the reference cursor of a counted record after its last op (64-bit), end' = min(end, ref_len).
 *   The record SPANS the step p -> p + 1 if pos <= p and p + 1 < end'; cover[p] is the number of counted records that span it
 *   (an N op spans like any other; the tools write none).  On the device: one u32 per position, the references back to back,
 *   +1 at pos and -1 at end' - 1 when end' - pos >= 2 (wrapping adds that return nothing), a prefix sum at bmn_finish.
 *
 *   EVENTS.  The ops of a counted record are walked with the reference cursor rc (from pos) and the query cursor qc (from 0).
 *   An I or D op of a length > 0 gives one event if
 *   - an M, =, X or D op of a length > 0 precedes it in the record (bmp.h's "anchored": a leading indel and one straight after
 *     S, H, P or N are dropped), and
 *   - rc >= 1; the anchor is a = rc - 1; and
 *   - for a D: rc + len <= ref_len;  for an I: rc < end', some reference base of this record follows inside the reference.
 *   An event is four u32: slot, w1, seq_lo, seq_hi.  slot is the anchor among the references back to back.  w1 = len |
 *   kind << 31 | other << 30 with DEL = 0, INS = 1 and len the 28-bit CIGAR length.  An I of len <= 32 whose 4-bit codes are
 *   all 1, 2, 4 or 8 has other = 0 and seq (seq_lo | seq_hi << 32) holds base j as 2 bits (A C G T = 0 .. 3) at bit 2 j; a
 *   longer I or one with another code has other = 1 and seq = 0; a D has seq = 0.
 *
 *   ALLELES.  The distinct events with their count n, ascending by (slot, w1, seq) as one 128-bit key.  An allele is
 *   BMN_ALLELE_WORDS = 8 u32: reference, anchor, w1, seq_lo, seq_hi, n, 0, 0.
 *
 *   SITES AND CALLS.  Per anchor that has events: E = the number of all its events; D = cover[a]; the ALT is the allele with
 *   other == 0 and the largest n, a tie goes to the first in allele order; n_alt = n(ALT); n_ref = D - E, saturating at 0 (a
 *   read with an I and a D on one anchor gives two events); n_oth = E - n_alt.  The anchor is a site if an ALT exists, D > 0,
 *   n_alt >= min_alt and, in u64, n_alt * 1 000 000 >= min_frac_ppm * D.  Costs in u64 centi-phred:
 *       L(RR) = 100 q_indel n_alt,   L(RA) = 301 (n_ref + n_alt) + prior,   L(AA) = 100 q_indel n_ref + prior;
 *   the other reads cost the same under all three and are left out.  The smallest wins; a tie goes to RR, then to RA.
 *   GQ = min(99, (the second smallest of the three, as a multiset, minus the least) / 100); qual = min(L(RR) - least,
 *   2^32 - 1); PL[k] = min(L(k) - least, 2^32 - 1), as in bmg.h.
 *   A call is BMN_CALL_WORDS = 16 u32: 0 reference, 1 anchor, 2 w1, 3 seq_lo, 4 seq_hi (of the ALT), 5 flags (bit 0 GENOTYPED,
 *   always set; bit 1 VARIANT: not RR), 6 the number of ALT copies 0 .. 2, 7 GQ, 8 qual, 9 n_ref, 10 n_alt, 11 n_oth (at most
 *   2^32 - 1), 12 DP = D, 13 .. 15 PL[RR, RA, AA].  Calls are listed in (reference, anchor) order.
 *
 * LEFT OUT, on purpose: more than one ALT per anchor; the base qualities of inserted bases; a homopolymer- or repeat-aware
 * error model; realignment of reads around a candidate; the overlap of two mates (unless the records were written with `--clip-overlap`); insertions above 32 bases as alleles (they
 * count as `other`); other ploidies and several samples; windows for genomes whose state does not fit.
 *
 * A context is used as bmn_begin, any number of bmn_add, bmn_finish, then any number of bmn_alleles / bmn_calls / bmn_cover_at;
 * bmn_events_of may be asked at any time after bmn_begin.  bmn_begin may be called again at any time and starts over.  The
 * state on the device is 4 bytes per base (cover) and 16 bytes per event; an add holds its stream and 16 bytes per record
 * beside it, and bmn_finish the sort's buffers, 24 bytes per event (two u64 keys, two u32 indices), and 12 more per event for
 * the heads, ranks and starts of the runs, 32 per allele and 64 per call.  Fewer than 2^31 events in one context.  What does
 * not fit is BMN_ERR_HIP with the sizes in the message.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMN_ERR_ARG, runs nothing and leaves the context
 * usable (after a refused bmn_add the records added before it are still there).
 *   bmn_begin: n_ref == 0, a length of 0, more bases than bmp_begin takes, min_alt == 0, min_frac_ppm > 1 000 000, q_indel
 *   == 0 or > 93, a null pointer.
 *   bmn_add: what bmp_add checks, in its order; the checks of the data need no context.  Then: no bmn_begin before it, or a
 *   bmn_finish since; refID >= n_ref on a record without flag 0x4.  n_records == 0 succeeds.
 *   bmn_finish: no bmn_begin before it, or a second bmn_finish; a null pointer.
 *   bmn_alleles / bmn_calls / bmn_cover_at: no bmn_finish before it; first + count beyond the list, ref >= n_ref, start +
 *   count beyond the reference; a null pointer with count > 0.
 *   bmn_events_of: no bmn_begin before it; add >= the number of bmn_add calls (when events are asked for); a null out_n_adds.
 *
 * Conventions as in bmp.h: plain C types, int status (the codes are BMS_*'s), message in bmn_last_error(), no CPU path.
 * bucket-map_amd/host/indel.h states the same rule in plain C++ and writes the VCF lines, tests/indel_rule.py in Python.
 */
#ifndef BMN_H
#define BMN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMN_OK = 0, BMN_ERR_ARG = 1, BMN_ERR_HIP = 2 };
enum { BMN_MIN_MAPQ = 0, BMN_MIN_ALT = 1, BMN_MIN_FRAC_PPM = 2, BMN_Q_INDEL = 3, BMN_PRIOR = 4, BMN_N_PARAMS = 5 };
enum { BMN_EVENT_WORDS = 4, BMN_ALLELE_WORDS = 8, BMN_CALL_WORDS = 16, BMN_N_STATS = 3, BMN_MAX_INS = 32 };
enum { BMN_GENOTYPED = 1, BMN_VARIANT = 2 };
enum { BMN_W_REF = 0, BMN_W_ANCHOR = 1, BMN_W_W1 = 2, BMN_W_SEQ = 3, BMN_W_FLAGS = 5, BMN_W_COPIES = 6, BMN_W_GQ = 7, BMN_W_QUAL = 8, BMN_W_NREF = 9,
       BMN_W_NALT = 10, BMN_W_NOTH = 11, BMN_W_DP = 12, BMN_W_PL = 13 };

typedef struct bmn_ctx bmn_ctx;

const char *bmn_last_error(void);
int  bmn_create(int32_t device, bmn_ctx **out);
void bmn_destroy(bmn_ctx *ctx);

/* Sizes the state for the n_ref references and zeroes it.  params points to the BMN_N_PARAMS values in the order above. */
int  bmn_begin(bmn_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params);

/* Adds the cover and the events of the counted records among the n_records records of in[0, n_bytes). */
int  bmn_add(bmn_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* Alleles, cover and calls of everything added: the three counts, and out_ref_stats[BMN_N_STATS * r + k] = n_reads,
 * n_low_mapq, n_left_out of reference r. */
int  bmn_finish(bmn_ctx *ctx, uint64_t *out_n_events, uint64_t *out_n_alleles, uint64_t *out_n_calls, uint64_t *out_ref_stats);

/* Alleles first .. first + count - 1, BMN_ALLELE_WORDS u32 each;  calls likewise, BMN_CALL_WORDS u32 each. */
int  bmn_alleles(bmn_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);
int  bmn_calls(bmn_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* For tests: *out_n_adds = the bmn_add calls with records since bmn_begin.  With out_n_events: the number of events the
 * call number `add` gave; with out_events also those events, unsorted, BMN_EVENT_WORDS u32 each, as the add wrote them (in
 * the order of its records, and of the ops inside a record). */
int  bmn_events_of(bmn_ctx *ctx, uint64_t add, uint64_t *out_n_adds, uint64_t *out_n_events, uint32_t *out_events);

/* cover[start .. start + count - 1] of reference ref. */
int  bmn_cover_at(bmn_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out);

/* Times in ms (HIP events on the context's stream): the passes of every bmn_add since bmn_begin, summed (they include the
 * host's read of the event count), and bmn_finish's sorts, scans and passes (with the host's reads of the digit counts and
 * the list sizes). */
int  bmn_last_stats(bmn_ctx *ctx, float *ms_add, float *ms_finish);

#ifdef __cplusplus
}
#endif
#endif
