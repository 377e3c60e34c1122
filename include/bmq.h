/*
 * bmq.h -- C ABI of the MI355X mapping statistics of a BAM record stream ("bucket-map QC", part of libbmf.so).
 *
 * With --stats FILE the tools say what the run was like: how many records mapped, as proper pairs, as duplicates; the insert
 * sizes; base quality, base composition and CIGAR classes along the read; GC; indel lengths.  Every other pass over the final
 * records (bmc.h, bmp.h, bmg.h, bmn.h, bmb.h, bmk.h) keeps its state per reference position; this is the one whose state is
 * indexed by READ CYCLE, so it has a walk and counters of its own.
 *
 * THE RULE IS EXACT, in integers only, and a function of the MULTISET of records and the two parameters: it does not depend on
 * the order of the records, on how they are cut over bmq_add calls, or on the grid.  The record layout is the BAM layout of
 * bms.h.  No reference sequence or length is needed.
 *
 *   PARAMETERS, two u32 in this order: max_cycle C (1 .. 65 535; --stats-max-cycle, 1024) and max_insert I (1 .. 65 535;
 *   --stats-max-insert, 8000).
 *
 *   CLASSES of a record that is not skipped (skip[i] == 0).  PRIMARY: neither 0x100 nor 0x800.  MAPPED: no 0x4.  PLACEHOLDER:
 *   the long-CIGAR placeholder of bmp.h (n_cigar_op == 2, the first op is l_seq S, the second an N).  ALIGNED: MAPPED,
 *   n_cigar_op > 0, l_seq > 0 and no PLACEHOLDER.  PAIRED: PRIMARY with 0x1.
 *
 *   TALLIES, BMQ_N_TALLIES = 35 u64 in this order: 0 records; 1 primary; 2 secondary (0x100); 3 supplementary (0x800);
 *   4 duplicates (0x400); 5 qc_failed (0x200); 6 mapped; 7 primary_mapped; 8 paired; 9 read1 (PAIRED with 0x40); 10 read2
 *   (PAIRED with 0x80); 11 properly_paired (PAIRED, 0x2, MAPPED); 12 both_mapped (PAIRED, MAPPED, no 0x8); 13 singletons
 *   (PAIRED, MAPPED, 0x8); 14 mate_other_ref (both_mapped and next_refID != refID); 15 mate_other_ref_mapq5 (the same with
 *   mapq >= 5); 16 reverse_strand (MAPPED with 0x10); 17 mapq0 (MAPPED with mapq == 0); 18 bases (the sum of l_seq over PRIMARY);
 *   19 bases_mapped (over PRIMARY and MAPPED); 20 aligned_records; 21 left_out (MAPPED with the PLACEHOLDER).
 *   Over the ops of ALIGNED records: 22 bases_m, 23 bases_eq, 24 bases_x (the lengths of M, = and X ops); 25 inserted bases;
 *   26 deleted bases; 27 soft-clipped bases; 28 insertions (I ops of a length > 0); 29 deletions (D ops of a length > 0).
 *   30 qual_sum and 31 qual_bases: the sum of the quality bytes and the number of the bases of PRIMARY records whose quality
 *   byte is not 0xFF, at every cycle.  32 bases_beyond_cycle, 33 pairs_in_is, 34 reads_no_acgt: below.
 *
 *   CYCLE.  The base at query index j of a record has the cycle c = j without 0x10 and c = l_seq - 1 - j with 0x10.  Its LETTER AS
 *   SEQUENCED is its 4-bit code without 0x10 and the complemented code with 0x10 (1 <-> 8, 2 <-> 4, every other code stays and
 *   is "other").  Hard clips do not shift cycles (a known departure).  A cell at c >= C is dropped; tally 32 counts the bases
 *   of PRIMARY records dropped that way from the BC table.
 *
 *   TABLES, all cells u64 at the ABI, rows x width:
 *   MAPQ [256] x 1    MAPPED records by mapq.
 *   RL   [C + 1] x 1  PRIMARY records by min(l_seq, C).
 *   IS   [I + 1] x 3  records with all of PRIMARY, 0x1, MAPPED, no 0x8, next_refID == refID and tlen > 0, by min(tlen, I);
 *                     column 0 inward (no 0x10, 0x20), column 1 outward (0x10, no 0x20), column 2 everything else.  Tally 33
 *                     counts these records.
 *   GC   [101] x 1    PRIMARY records with l_seq > 0: n the bases of code 1, 2, 4 or 8, g those of code 2 or 4; with n == 0
 *                     the record goes to tally 34 and nowhere here, else to row (200 g + n) / (2 n), the percentage rounded
 *                     half up.
 *   ID   [256] x 2    the I (column 0) and D (column 1) ops of a length > 0 of ALIGNED records, by min(length, 255).
 *   BC   [C] x 5      the letters as sequenced (A C G T other) of PRIMARY records, by cycle.
 *   QC   [C] x 64     the bases of PRIMARY records whose quality byte q is not 0xFF, by cycle and min(q, 63).
 *   MC   [C] x 6      the bases of ALIGNED records by cycle and the op that holds them: columns =, X, M, I, S, D.  A D op of a
 *                     length > 0 counts once, at the cycle of the query index qc - 1, where qc is the query cursor when the op
 *                     is met; it is dropped if qc == 0.  N, H and P add nothing.
 *
 * LEFT OUT, on purpose: NM/MD and any other tag; read groups; counts per reference (--coverage has them); counts per tile or
 * lane; GC against depth; any threshold on mapq or quality; secondary and supplementary records in the read-level tables;
 * compatibility of the text file with another tool's parser (the section names are borrowed, the meaning is the one written
 * here).
 *
 * A context is used as bmq_begin, any number of bmq_add, bmq_finish, then bmq_table in any order; bmq_begin may be called again
 * at any time and starts over.  The state on the device is 600 bytes per cycle, 24 bytes per insert size and a few KB.
 * BMQ_LDS_CYCLES=n in the environment, read at bmq_create, forces the number of cycles whose counters a workgroup keeps in LDS
 * (0: every cell by global atomics; more than BMQ_MAX_LDS_CYCLES counts as that); it changes no output.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each returns BMQ_ERR_ARG, runs nothing and leaves the context usable
 * (after a refused bmq_add the records added before it are still there).
 *   bmq_begin: a null pointer; C or I outside 1 .. 65 535.
 *   bmq_add: what bmp_add checks, in its order -- the stream itself, an op code above 8, the query length against l_seq, null
 *   pointers; there is no test of refID, because there are no references; the checks of the data need no context -- then no
 *   bmq_begin before it, or a bmq_finish since.  n_records == 0 succeeds.
 *   bmq_finish: no bmq_begin before it, or a bmq_finish since.
 *   bmq_table: no bmq_finish before it; an unknown table; first + count beyond the table's rows; a null pointer with
 *   count > 0.
 *
 * Conventions as in bmk.h: plain C types, int status (the codes are BMS_*'s), message in bmq_last_error(), no CPU path.
 * bucket-map_amd/host/stats.h states the same rule in plain C++ and writes the text, tests/stats_rule.py in Python.
 */
#ifndef BMQ_H
#define BMQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMQ_OK = 0, BMQ_ERR_ARG = 1, BMQ_ERR_HIP = 2 };
enum { BMQ_MAX_CYCLE = 0, BMQ_MAX_INSERT = 1, BMQ_N_PARAMS = 2 };
enum { BMQ_N_TALLIES = 35, BMQ_N_TABLES = 8, BMQ_MAX_LDS_CYCLES = 512 };
enum { BMQ_T_MAPQ = 0, BMQ_T_RL = 1, BMQ_T_IS = 2, BMQ_T_GC = 3, BMQ_T_ID = 4, BMQ_T_BC = 5, BMQ_T_QC = 6, BMQ_T_MC = 7 };
enum {
    BMQ_RECORDS = 0, BMQ_PRIMARY = 1, BMQ_SECONDARY = 2, BMQ_SUPPLEMENTARY = 3, BMQ_DUPLICATES = 4, BMQ_QC_FAILED = 5, BMQ_MAPPED = 6,
    BMQ_PRIMARY_MAPPED = 7, BMQ_PAIRED = 8, BMQ_READ1 = 9, BMQ_READ2 = 10, BMQ_PROPERLY_PAIRED = 11, BMQ_BOTH_MAPPED = 12, BMQ_SINGLETONS = 13,
    BMQ_MATE_OTHER_REF = 14, BMQ_MATE_OTHER_REF_MAPQ5 = 15, BMQ_REVERSE_STRAND = 16, BMQ_MAPQ0 = 17, BMQ_BASES = 18, BMQ_BASES_MAPPED = 19,
    BMQ_ALIGNED_RECORDS = 20, BMQ_LEFT_OUT = 21, BMQ_BASES_M = 22, BMQ_BASES_EQ = 23, BMQ_BASES_X = 24, BMQ_INSERTED_BASES = 25,
    BMQ_DELETED_BASES = 26, BMQ_SOFT_CLIPPED_BASES = 27, BMQ_INSERTIONS = 28, BMQ_DELETIONS = 29, BMQ_QUAL_SUM = 30, BMQ_QUAL_BASES = 31,
    BMQ_BASES_BEYOND_CYCLE = 32, BMQ_PAIRS_IN_IS = 33, BMQ_READS_NO_ACGT = 34
};

typedef struct bmq_ctx bmq_ctx;

const char *bmq_last_error(void);

int  bmq_create(int32_t device, bmq_ctx **out);
void bmq_destroy(bmq_ctx *ctx);

/* Sizes the tables for the BMQ_N_PARAMS values of params and zeroes them and the tallies. */
int  bmq_begin(bmq_ctx *ctx, const uint32_t *params);

/* Counts the records that are not skipped among the n_records records of in[0, n_bytes); skip may be null. */
int  bmq_add(bmq_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip);

/* Everything added is in the tables; out_tallies (may be null) receives the BMQ_N_TALLIES u64. */
int  bmq_finish(bmq_ctx *ctx, uint64_t *out_tallies);

/* Rows first .. first + count - 1 of table `which` (BMQ_T_*), row-major, after bmq_finish.  The tables have 256, C + 1, I + 1,
 * 101, 256, C, C and C rows of 1, 1, 3, 1, 2, 5, 64 and 6 u64. */
int  bmq_table(bmq_ctx *ctx, uint32_t which, uint64_t first, uint64_t count, uint64_t *out);

/* Times in ms (HIP events on the context's stream): the kernels of every bmq_add since bmq_begin, summed, and the work of the
 * last bmq_finish on the device. */
int  bmq_last_stats(bmq_ctx *ctx, float *ms_add, float *ms_finish);

#ifdef __cplusplus
}
#endif
#endif
