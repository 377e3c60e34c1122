// bmv_realign.hip.h -- the affine-gap realignment pass of the verifier (bmv_realign, include/bmv.h): a banded Gotoh
// recurrence that follows an alignment's edit path, and its traceback.  A post-pass of its own: no aligning kernel is touched.
//
// Shape: a wave per alignment, a lane per band column of the current row, the wave stepping row by row.  Lane c of row i
// is column base(i) + c with base(i) = p(i) - band (signed: the band may hang over the text's start), so the band's left
// edge moves by shift(i) = p(i) - p(i-1) = (the D run that followed row i-1) + (1 when row i is entered by an M column).
// The wave walks the CIGAR in uniform registers to know that shift; the upper and diagonal predecessors are then lanes
// c + shift and c + shift - 1 of the row before: two shuffles with a uniform offset (H and Ins), the diagonal one being the
// upper one of the lane to the left; no table of band starts.
// The Del chain of a row is a dependency across lanes, resolved as a prefix maximum:
//   Del(c) = max over c' < c of (H'(c') + c' ext) - open - c ext,   H' = max(diagonal, Ins)
// (opening from a Del-derived H is strictly worse than extending because gap_open >= 1): six steps.  The open / extend
// code of a Del cell is then read off its left neighbour's H and Del, as the recurrence states it.  The scan and every
// move from the left neighbour are DPP operations on the VALU (row_shr, row_bcast:15 / :31, wave_shr:1): as ds_bpermute
// shuffles they made 14 LDS-pipe operations a row and the pipe the limit (profiles/r10/README.md); three remain.
// Absent cells hold kAbsent, far enough below every score a present cell can have (the host checks the bound) that sums of
// it with a few penalties stay below kFloor; whatever falls below kFloor is made kAbsent again, so an absent operand never
// wins a maximum and nothing drifts.
// Text ranks sit in three registers of 64 columns each (the current one, the next, and one on its way), the lane's base
// comes out of the first two by one shuffle of both; query ranks in two registers, the row's base read by its lane number.
// Per row one coalesced store of 64 direction bytes: bits 0-1 the source of H (0 diagonal, 1 Ins, 2 Del), bit 2 Ins
// extends, bit 3 Del extends; the row's shift rides in the high nibbles of bytes 0 and 1.
// The traceback is a kernel of its own: a wave pulls 64 rows of codes (4 KB) into LDS and walks them, all lanes in step
// (the walk is uniform), writing run-length entries in reversed order; a scan (bm_scan.hip.h) and a gather put them in
// order at packed offsets.  An alignment that is passed through (a D entry too long for the band, an empty CIGAR) takes
// the other branch of the forward kernel: one walk along the given path for its affine score, a ballot of "ranks differ"
// per 64 columns of an M entry; the gather copies its entries as they came.
#pragma once

#include "bm_dna4.hip.h"

namespace bmv {

constexpr int32_t kFloor = -(1 << 30);                   // every present cell lies above this (checked on the host)
constexpr int32_t kAbsent = kFloor - (1 << 20);          // an absent cell; +- a few penalties it stays below kFloor

struct RealignJob {
    const uint8_t *genome;
    const uint8_t *reads;
    const uint64_t *text_start;     // per alignment of the batch
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    const uint32_t *begin;
    const uint64_t *cigar_offset;   // n + 1
    const uint32_t *cigar;          // M / I / D, validated on the host
    const uint8_t *pass;            // 1: passed through (decided on the host from the entries)
    const uint64_t *row_at;         // a realigned alignment's first row of codes, counted in rows from the piece's first
    const uint64_t *ops_at;         // ... and its first reversed entry
    uint32_t first, count;          // the piece: alignments first .. first + count - 1
    int32_t match, mismatch, open, ext;
    uint32_t band;
    uint8_t *codes;                 // 64 bytes a row
    uint32_t *ops_rev;
    int32_t *score;                 // per alignment of the batch
    uint32_t *out_begin, *end_lane, *nops;
    const uint64_t *out_offset;     // the gather: the piece's packed offsets (count + 1) ...
    uint32_t *out_cigar;            // ... and entries
};

// defined in bmv_realign.hip; one wave a block, a block an alignment of the piece (the gather: eight threads an alignment)
__global__ void bmv_realign_forward_kernel(RealignJob J);
__global__ void bmv_realign_trace_kernel(RealignJob J);
__global__ void bmv_realign_gather_kernel(RealignJob J);

}  // namespace bmv
