// bmv_leftalign.hip.h -- the indel normalisation pass of the verifier (bmv_leftalign, include/bmv.h): every I and D entry of
// a known M/I/D path moved to its leftmost equivalent place on the forward strand.  A post-pass of its own: no aligning
// kernel is touched.
//
// Shape: a wave per alignment walks the entries in FORWARD-strand order (for text_rc != 0 from the last entry to the first,
// the query read from its last base to its first; both sides of every comparison come from the same sequence, so no rank is
// complemented) with the cursors, the gap under way and the top of the output stack in uniform registers.  Entries are
// fetched 64 at a time, one a lane, and read by lane number.  The stack's body lies in a slot of E + (gap entries) words of
// the scratch, written and read back by lane 0 alone -- a pop is then a load by the thread that stored.
// A gap of length L in front of an M run of k columns: lane t - 1 loads the two bytes L apart that shift t compares (from the
// genome for a D, from the read for an I; 64 neighbouring bytes each), one ballot of "equal" and a count of trailing ones
// give up to 64 columns of shift a step, and the wave goes on while all 64 lanes hold and the run lasts.
// The stack of a forward-strand alignment is its output; a gather (bmv_leftalign_gather_kernel) puts the entries in the
// aligner's order at the packed offsets a scan of the counts gives (bm_scan.hip.h).
#pragma once

#include "bm_dna4.hip.h"

namespace bmv {

constexpr uint32_t kLeftAlignWaves = 4;         // alignments per 256-thread block

struct LeftAlignJob {
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
    const uint64_t *slot_at;        // an alignment's stack slot, counted in words from the piece's first
    uint32_t first, count;          // the piece: alignments first .. first + count - 1
    uint32_t *stack;
    uint32_t *out_begin, *nops, *dropped, *merges;   // per alignment of the batch
    uint64_t *compared;
    uint8_t *changed;
    const uint64_t *out_offset;     // the gather: the piece's packed offsets (count + 1) ...
    uint32_t *out_cigar;            // ... and entries
};

// defined in bmv_leftalign.hip; kLeftAlignWaves waves a block, a wave an alignment of the piece (the gather: eight threads an
// alignment)
__global__ void bmv_leftalign_kernel(LeftAlignJob J);
__global__ void bmv_leftalign_gather_kernel(LeftAlignJob J);

}  // namespace bmv
