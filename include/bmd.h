/*
 * bmd.h -- C ABI of the MI355X duplicate marker ("bucket-map duplicates", part of libbmf.so).
 *
 * With --markdup the tools' BAM stream has its duplicate reads flagged (0x400) on the device between the upload and the
 * coordinate sort of bms.h: the marker needs every record before any is written and needs them in the order the tool wrote
 * them, where mates are adjacent -- which is what the sorter holds and what is lost after it.
 *
 * THE RULE IS EXACT, in integers only, and a function of the record stream alone.
 *   A record is rec_offset[i] .. rec_offset[i + 1] of a BAM stream, as in bms.h.  Its fields, little-endian, at offsets from
 *   the record's start: block_size 0, refID (i32) 4, pos (i32) 8, l_read_name (u8) 12, n_cigar_op (u16) 16, flag (u16) 18,
 *   l_seq (u32) 20, the name 36; then n_cigar_op u32 ops (length << 4 | op, op = MIDNSHP=X as 0..8), then (l_seq + 1) / 2
 *   sequence bytes, then l_seq quality bytes.
 *
 *   Per record i:
 *   - reflen = the sum of the M, D, N, =, X op lengths; lead / trail = the summed lengths of the leading / trailing run of
 *     S and H ops (a CIGAR of clips only is both runs at once; no CIGAR: reflen = lead = trail = 0).
 *   - end5(i), the unclipped 5' coordinate: pos - lead without flag 0x10, pos + reflen + trail - 1 with it.
 *   - eligible(i): flag has none of 0x4, 0x100, 0x800; refID >= 0; the CIGAR is not the long-CIGAR placeholder
 *     (n_cigar_op == 2, op 0 is l_seq S, op 1 is an N); end5 lies in [-2^31, 2^31).
 *   - E(i) = (uint64)refID << 33 | (uint64)(end5 + 2^31) << 1 | reverse   (reverse = flag 0x10).
 *   - score(i) = the sum, a uint64, of the quality bytes q with 15 <= q and q != 0xFF.
 *
 *   Mates: records i and i + 1 are mates when both have 0x1, neither has 0x100 or 0x800, i has 0x40 and not 0x80, i + 1 has
 *   0x80 and not 0x40, and their l_read_name and name bytes are equal.  The first of a pair is always the 0x40 record, so no
 *   chains arise and nothing depends on a left-to-right scan (--paired writes records 2p and 2p + 1 this way).
 *
 *   kind(i): 0 not eligible.  2 and 3: i and i + 1 are mates and both eligible -- a PAIR UNIT with the 128-bit key
 *   (min(E_i, E_i+1), max(E_i, E_i+1)) and the score score_i + score_i+1.  1: every other eligible record -- a FRAGMENT UNIT
 *   with key E and its own score.
 *
 *   Marking:
 *   - among pair units of equal key the one with the greatest score is kept, ties to the lowest i; both records of every
 *     other one are duplicates;
 *   - a fragment unit is a duplicate if any pair unit has an end (either one) with the same E;
 *   - otherwise, among fragment units of equal E, the one with the greatest score is kept, ties to the lowest i; the others
 *     are duplicates;
 *   - nothing else is a duplicate.
 *   A duplicate gets 0x400 ORed into its flag: bit 2 of the byte at record offset 19.  No other byte of any record changes.
 *
 *   This is Picard's / samtools markdup's rule with sum-of-base-qualities scoring.  KNOWN DEPARTURES, ours:
 *   - supplementary records are never marked;
 *   - records with a long-CIGAR placeholder are never marked;
 *   - there is no optical-duplicate distance;
 *   - there are no library or read-group keys.
 *   bucket-map_amd/host/markdup.h states the same rule in plain C++, tests/markdup_rule.py in Python.
 *
 * bmd_mark_sort_deflate uploads the stream once, computes the descriptors, marks, sets the flag bytes in the device copy and
 * then runs bms_sort_deflate's sort, gather and deflate on it: the output is exactly bms_sort_deflate of the stream with the
 * flags set, and the marked stream never leaves the device unsorted.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMD_ERR_ARG, runs nothing and leaves the context
 * usable.  bmd_ends and bmd_mark_sort_deflate: everything bms_sort / bms_sort_deflate check of the stream (bms.h), and a
 * record whose name, CIGAR, sequence and qualities do not fit inside its extent
 * (36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > length).  bmd_mark: n > 2^31 - 1; a kind above 3; a 2 not
 * followed by a 3 or a 3 not preceded by a 2.  A null pointer (arrays of n_records elements may be null when there are none).
 * The context is looked at last, so the checks of the data need no device.  n = 0 succeeds.  A failed allocation returns
 * BMD_ERR_HIP with the sizes in the message.
 *
 * Conventions as in bms.h: plain C types, int status, message in bmd_last_error(), no CPU path.
 */
#ifndef BMD_H
#define BMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMD_OK = 0, BMD_ERR_ARG = 1, BMD_ERR_HIP = 2 };

typedef struct bmd_ctx bmd_ctx;

const char *bmd_last_error(void);
int  bmd_create(int32_t device, bmd_ctx **out);
void bmd_destroy(bmd_ctx *ctx);

/* The descriptors of the n_records records of in[0, n_bytes): out_end[i] = E(i) (0 for kind 0), out_score[i] = score(i)
 * (the sum also for kind 0), out_kind[i] = kind(i). */
int  bmd_ends(bmd_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records,
              uint64_t *out_end, uint64_t *out_score, uint8_t *out_kind);

/* Marks from descriptors of any origin (several runs concatenated, say): out_dup[i] = 1 for a duplicate, else 0.
 * out_counts = pair units, fragment units, duplicate records from pair units, duplicate fragment records. */
int  bmd_mark(bmd_ctx *ctx, const uint64_t *end, const uint64_t *score, const uint8_t *kind, uint64_t n, uint8_t *out_dup,
              uint64_t *out_counts);

/* bms_sort_deflate (its arguments, its output) of the stream with 0x400 set in the duplicates' flags; out_dup and out_counts
 * as bmd_mark, in the order of the input. */
int  bmd_mark_sort_deflate(bmd_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records,
                           uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *out_perm,
                           uint64_t *out_sorted_offset, uint8_t *out_dup, uint64_t *out_counts);

/* The last call's times in ms (HIP events on the context's stream): the descriptors (0 after bmd_mark), the marking (0 after
 * bmd_ends; it includes the host's reads of the digit counts), and the radix passes the marking ran (0 .. 40). */
int  bmd_last_stats(bmd_ctx *ctx, float *ms_ends, float *ms_mark, uint32_t *n_passes);

/* bms_last_stats of the sort, gather and deflate that bmd_mark_sort_deflate ran after the marking (0 after the other calls). */
int  bmd_last_sort_stats(bmd_ctx *ctx, float *ms_sort, float *ms_gather, float *ms_deflate, uint32_t *n_passes);

#ifdef __cplusplus
}
#endif
#endif
