/*
 * bmc.h -- C ABI of the MI355X coverage counter ("bucket-map coverage", part of libbmf.so).
 *
 * With --depth / --coverage the tools report, for the BAM records they have just written, how deep every base of every
 * reference is covered and how much of each reference is covered at all: the records are still at hand when the file is
 * done (the sorter of bms.h holds them), so no second program has to read and inflate the file again.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of counted records: it does not depend on the order
 * of the records, on how they are cut over bmc_add calls, or on the grid.
 *   A record is rec_offset[i] .. rec_offset[i + 1] of a BAM stream, as in bms.h / bmd.h.  Its fields, little-endian, at
 *   offsets from the record's start: block_size 0, refID (i32) 4, pos (i32) 8, l_read_name (u8) 12, mapq (u8) 13,
 *   n_cigar_op (u16) 16, flag (u16) 18, l_seq (u32) 20, the name 36; then n_cigar_op u32 ops (length << 4 | op,
 *   op = MIDNSHP=X as 0..8), then (l_seq + 1) / 2 sequence bytes, then l_seq quality bytes.
 *   References 0 .. n_ref - 1 have lengths ref_len[r] (u32, each >= 1).  skip[i] is an optional byte per record.
 *
 *   COUNTED RECORD.  Record i is PLACED when
 *   - its flag has none of 0x4, 0x100, 0x200, 0x400 (supplementary records, 0x800, are placed);
 *   - skip is null or skip[i] == 0;
 *   - 0 <= refID < n_ref and 0 <= pos < ref_len[refID];
 *   - n_cigar_op > 0.
 *   A placed record is COUNTED unless its CIGAR is the long-CIGAR placeholder (n_cigar_op == 2, op 0 is l_seq S, op 1 is an
 *   N, as in bmd.h); a placed record with the placeholder is LEFT OUT and adds one to n_long of its reference, nothing else.
 *   KNOWN DEPARTURE, the same as the marker's: the real CIGAR of such a record (its CG:B,I tag) is not read.
 *
 *   BLOCKS.  The ops of a counted record are walked with a reference cursor that starts at pos and a query cursor that
 *   starts at 0 (both 64-bit): M, = and X advance both and each forms the block [reference cursor, reference cursor + len);
 *   D and N advance the reference cursor only; I and S the query cursor only; H and P neither.  A block is clipped to
 *   [0, ref_len[refID]): what lies beyond the end of the reference is not counted, and its query bases are not either.
 *
 *   DEPTH.  depth(r, p) = the number of (clipped) blocks of counted records on r that hold p.  D and N do not count, mates
 *   that overlap count twice (unless the records were written with `--clip-overlap`, which soft-clips the overlap away), and
 *   there is no base-quality or MAPQ threshold.
 *
 *   RUNS.  Per reference in ascending order, the maximal intervals [start, end) of equal depth > 0, as (r, start, end,
 *   depth): references ascending, starts ascending.  A run never spans two references.
 *
 *   PER REFERENCE, seven u64: n_reads (the counted records on it), cov_bases (positions with depth > 0), sum_depth (over its
 *   positions), sum_mapq (over its counted records), sum_qual and n_qual (the sum and the number of the quality bytes
 *   q != 0xFF of the query bases inside the clipped blocks; a record with l_seq == 0 adds to neither), n_long.
 *
 * A context is used as bmc_begin, any number of bmc_add, bmc_finish, then any number of bmc_runs / bmc_depth_at; bmc_begin
 * may be called again at any time and starts over (nothing of the earlier references or records remains).  The state on the
 * device is one 32-bit difference array over the references back to back, each with one slot more than it has bases, and its
 * prefix sum: 8 bytes per base.  What does not fit into free device memory is BMC_ERR_HIP (windows are out of scope).
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMC_ERR_ARG, runs nothing and leaves the context
 * usable (after a refused bmc_add the records added before it are still there).
 *   bmc_begin: n_ref == 0, a length of 0, more than 2^32 - 2^20 bases in all (or, with the references' extra slots, 2^32 - 1
 *   slots or more), a null pointer.
 *   bmc_add: everything bmd_ends checks of the stream (bms.h, and the fields of every record lie inside it); an op code above
 *   8; n_cigar_op > 0, l_seq != 0 and the summed M, I, S, =, X lengths differ from l_seq; a null pointer (skip may be null;
 *   in and rec_offset's companions may be null when there is nothing); these need no context.  Then, with the context:
 *   no bmc_begin before it, or a bmc_finish since; refID >= n_ref on a record without flag 0x4.  n_records == 0 succeeds.
 *   bmc_finish: no bmc_begin before it, or a second bmc_finish; a null pointer.
 *   bmc_runs / bmc_depth_at: no bmc_finish before it; first + count beyond the runs, ref >= n_ref, start + count beyond the
 *   reference; a null pointer with count > 0.
 * The context is looked at last, so the checks of the data need no device.  A failed allocation returns BMC_ERR_HIP with
 * the sizes in the message.
 *
 * Conventions as in bms.h: plain C types, int status, message in bmc_last_error(), no CPU path.
 * bucket-map_amd/host/depth.h states the same rule in plain C++, tests/depth_rule.py in Python.
 */
#ifndef BMC_H
#define BMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMC_OK = 0, BMC_ERR_ARG = 1, BMC_ERR_HIP = 2 };
enum { BMC_N_READS = 0, BMC_COV_BASES = 1, BMC_SUM_DEPTH = 2, BMC_SUM_MAPQ = 3, BMC_SUM_QUAL = 4, BMC_N_QUAL = 5, BMC_N_LONG = 6, BMC_N_STATS = 7 };

typedef struct bmc_ctx bmc_ctx;

const char *bmc_last_error(void);
int  bmc_create(int32_t device, bmc_ctx **out);
void bmc_destroy(bmc_ctx *ctx);

/* Sizes the state for the n_ref references and zeroes it. */
int  bmc_begin(bmc_ctx *ctx, const uint32_t *ref_len, uint32_t n_ref);

/* Adds the blocks of the counted records among the n_records records of in[0, n_bytes). */
int  bmc_add(bmc_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* Depths, runs and sums of everything added: *out_n_runs, and out_ref_stats[BMC_N_STATS * r + k] in the order above. */
int  bmc_finish(bmc_ctx *ctx, uint64_t *out_n_runs, uint64_t *out_ref_stats);

/* Runs first .. first + count - 1 as (reference, start, end, depth): out[4 * k .. 4 * k + 3]. */
int  bmc_runs(bmc_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* depth(ref, start) .. depth(ref, start + count - 1). */
int  bmc_depth_at(bmc_ctx *ctx, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out);

/* Times in ms (HIP events on the context's stream): the kernels of every bmc_add since bmc_begin, summed, and bmc_finish's
 * scans and passes (it includes the host's read of the run count). */
int  bmc_last_stats(bmc_ctx *ctx, float *ms_add, float *ms_finish);

#ifdef __cplusplus
}
#endif
#endif
