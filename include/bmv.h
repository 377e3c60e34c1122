/*
 * bmv.h -- C ABI of the MI355X alignment verifier ("bucket-map verify", part of libbmf.so).
 *
 * the `bucketmap_align` build of the reference (BM_ALIGN, CMakeLists.txt:138) sends
 * every located candidate through a SeqAn3 pairwise alignment before it is written to the SAM file:
 *
 *   reference (bucket_map/locator/bucket_locator.h)               this ABI
 *   ------------------------------------------------------------  -------------------------------------
 *   align_config: method_global, sequence1 end gaps free,         the only configuration the kernel has
 *     edit_scheme, output score/begin/alignment       :520-528
 *   text window = bucket_seq[bucket][offset, +width)  :549-550    (text_start, text_len) views, chosen by
 *   reverse complement of the text for strand 16      :562-567      the caller; text_rc
 *   align_pairwise(text, query)                       :569        bmv_align, all candidates in one batch
 *     (query.size() and the window of any width)      :549-589    bmv_align_long, beyond max_query_len / max_text_len
 *   alignment.score(), sequence1_begin_position(),    :570-576    out_score, out_begin, CIGAR entries
 *     cigar_from_alignment
 *
 * What stays on the host (bucket-map_amd/host/bucket_locator.h): the window arithmetic (:550), the
 * MAPQ = 60 + score rule and its threshold (:570-573), SAM output.
 *
 * Semi-global edit distance (the whole query against the best substring of the text, unit costs) by
 * Myers' bit-vector recurrence in words of 64 query rows: a query of up to 512 bases is one lane's work (64 alignments per
 * wave), a longer one is spread over a group of lanes skewed along the text (beyond 32 768 bases in strips of that many
 * rows); the traceback runs on the device too.  The score is unique; between equally good alignments SeqAn3's own choice is not
 * pinned by anything in the reference (no test, no fixture, SeqAn3 itself absent), so the rules are stated
 * here and a maintainer with SeqAn3 at hand can correct them in one place:
 *   (1) the alignment ends at the LAST text column whose bottom-row score is the minimum;
 *   (2) the traceback prefers the diagonal predecessor, then the upper one (a query base against a gap,
 *       CIGAR I), then the left one (a text base against a gap, CIGAR D);
 *   (3) CIGAR alphabet M / I / D (cigar_from_alignment without extended_cigar).
 *
 * Conventions as in bmf.h: plain C types, int status, message in bmv_last_error(), no CPU fallback.
 */
#ifndef BMV_H
#define BMV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMV_OK = 0, BMV_ERR_ARG = 1, BMV_ERR_HIP = 2, BMV_ERR_STATE = 3, BMV_ERR_UNSUPPORTED = 5 };

/* CIGAR entries are packed as in BAM: length << 4 | op. */
enum { BMV_OP_M = 0, BMV_OP_I = 1, BMV_OP_D = 2, BMV_OP_S = 4, BMV_OP_EQ = 7, BMV_OP_X = 8 };
/* = and X: the output of bmv_annotate and bmv_clip only; S (a soft clip): bmv_clip's output only */

typedef struct bmv_params {
    uint32_t max_query_len;   /* longest read handed to bmv_align (<= 65536)                        */
    uint32_t max_text_len;    /* longest text window: max_query_len + 1 + indel allowance (<= 81920) */
    int32_t  device;
} bmv_params;

typedef struct bmv_ctx bmv_ctx;

const char *bmv_last_error(void);
int  bmv_create(const bmv_params *params, bmv_ctx **out);
void bmv_destroy(bmv_ctx *ctx);

/* The reference genome as one byte string (ASCII; the same string bml_load_genome takes).  Uploaded once;
 * text windows are views into it. */
int  bmv_load_genome(bmv_ctx *ctx, const uint8_t *bases, uint64_t n_bases);
/* ... or from records that are buffers of their own on the host (concatenated on the device, in order; bml_load_genome_records). */
int  bmv_load_genome_records(bmv_ctx *ctx, const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records);

/* One batch of alignments: alignment a aligns the query reads[query_start[a], +query_len[a]) against the
 * text genome[text_start[a], +text_len[a]), reverse-complemented first when text_rc[a] != 0.  `reads` is
 * n_read_bytes of ASCII bases (dna4 folding as in bmf.h).  Results stay on the device until
 * bmv_results; *total_cigar receives the number of CIGAR entries of the whole batch. */
int  bmv_align(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
               const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start,
               const uint32_t *query_len, uint32_t n, uint64_t *total_cigar);

/* The same batch without the context's limits: any lengths that fit uint32.  Alignments within max_query_len and
 * max_text_len go through bmv_align itself (the same kernels, bit-identical results); longer ones through tiles of
 * 64 lanes x 8 words (32 768 query rows) x up to 8 192 text columns launched by anti-diagonal, with checkpoints in
 * the scratch (about 1.25 B per 64-row word and text column) and a traceback with the same tie rules.  The long ones
 * are taken in pieces that fit the scratch; one whose trace alone does not fit fails the call with BMV_ERR_UNSUPPORTED
 * (the message names it and the bytes it needs) before anything runs, and the context stays usable.  Results through
 * bmv_results / bmv_last_stats as for bmv_align.  BMV_LONG_FROM=<bases> (experiments, tests): every query of at least
 * that many bases takes the long path. */
int  bmv_align_long(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                    const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start,
                    const uint32_t *query_len, uint32_t n, uint64_t *total_cigar);

/* The same batch under an edit bound per alignment: alignment a is ACCEPTED iff its semi-global edit distance is at most
 * max_edits[a] -- exactly, not as a heuristic.  An accepted alignment has the score, begin and CIGAR bmv_align (or
 * bmv_align_long) gives it, bit for bit; a rejected one has score BMV_REJECTED, begin 0 and no CIGAR entries (its two offsets
 * are equal), and *total_cigar counts accepted entries only.  Argument checks and error codes are bmv_align_long's, so
 * lengths beyond the context's limits are allowed.
 * How: a score-only screen (bmv_screen_* kernels: the same recurrence with Ukkonen's cut-off at the lower end of the
 * column, no checkpoints, no traceback) rejects what it can prove to lie beyond its bound after the top-left corner of its
 * matrix; the survivors are aligned as a batch of their own by the unchanged kernels and the bound is applied to their
 * scores.  max_edits[a] >= query_len[a] can reject nothing and skips the screen.  Alignments beyond max_query_len /
 * max_text_len (or from BMV_LONG_FROM on) skip the screen too and take the bmv_align_long path: the same contract, no
 * saving. */
#define BMV_REJECTED INT32_MIN
int  bmv_align_bounded(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                       const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start,
                       const uint32_t *query_len, const uint32_t *max_edits, uint32_t n, uint64_t *total_cigar);
/* Of the last bmv_align_bounded: how many alignments were rejected, 64 x the (64-row word, text column) steps the screen
 * evaluated summed over alignments, and the screen's kernel time in ms (part of bmv_last_stats' ms_kernels, which covers
 * the whole call). */
int  bmv_last_bounded_stats(bmv_ctx *ctx, uint32_t *n_rejected, uint64_t *screen_cells, float *ms_screen);

/* The best alignment of each GROUP of a batch: one full alignment per group instead of one per alignment.  A group is the set of
 * candidate alignments of one read; group g owns the alignments group_offset[g] .. group_offset[g + 1] - 1 of the batch
 * (n_groups + 1 entries, non-decreasing, [0] = 0, [n_groups] = n).  The contract is on the outputs, exact, and independent of hint:
 *   d[a]                alignment a's semi-global edit distance: -score of bmv_align_long
 *   end[a]              begin + R of the result bmv_align_long gives it (R: its M and D lengths): the exclusive end column in
 *                       the text as the aligner saw it -- tie rule (1) above
 *   best[g]             the minimum of d over the group
 *   out_winner[g]       the LOWEST batch index a of the group with d[a] = best[g]; BMV_BEYOND for an empty group
 *   bmv_results         the winner carries exactly bmv_align_long's score, begin and CIGAR; every other alignment has score
 *                       BMV_REJECTED, begin 0 and no CIGAR entries; *total_cigar counts the winners' entries
 *   out_edits[a], out_end[a]   d[a] and end[a] whenever d[a] <= best[g] + margin[g] (the sum in 64 bits, capped at query_len[a]:
 *                       no distance is larger), else BMV_BEYOND and 0.  The winner is always within the margin.
 * hint[g] (or NULL: 0) is the index INSIDE group g of the alignment to try first -- the caller's guess at the winner; it decides
 * how much work the call is, never what it returns.  Argument checks and limits are bmv_align_long's; in addition group_offset
 * must be as above and hint[g] smaller than the group's size (ignored for an empty group): BMV_ERR_ARG, the message names the
 * group, nothing ran and the context stays usable.  The call leaves untouched what bmv_annotations, bmv_clipped and their stats
 * calls return, and everything else outside its row of the table above bmv_results (bmv_last_bounded_stats included).
 * How (bmv_best.hip.h): the hinted alignment of every group is aligned in full by bmv_align_long (a group of one is finished
 * there); every other one goes through score-only kernels -- bmv_align_bounded's screen made to decide: under
 * k = min(hinted edits + margin, query_len) they give the exact (d, end), or the proof that d > k, or give up when the band
 * outgrows a wave, and what they give up on (and what lies beyond the context's limits) is aligned in full; a segmented pass
 * picks the winners; the winners that were not aligned yet are aligned in full. */
#define BMV_BEYOND UINT32_MAX
int  bmv_align_best(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                    const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                    uint32_t n, const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                    uint64_t *total_cigar);
/* Of the last bmv_align_best: out_winner n_groups entries, out_edits and out_end n entries; any pointer may be NULL. */
int  bmv_best(bmv_ctx *ctx, uint32_t *out_winner, uint32_t *out_edits, uint32_t *out_end);
/* Of the last bmv_align_best: the alignments aligned in full as seeds, those that entered the distance round, of these the ones
 * proven beyond k and the ones given up on, the winners aligned in full after the pick, 64 x the (64-row word, text column)
 * steps of the distance round (as screen_cells), and the kernel ms of the distance round and of the pick (parts of
 * bmv_last_stats' ms_kernels, which covers the whole call).  Any pointer may be NULL. */
int  bmv_last_best_stats(bmv_ctx *ctx, uint32_t *n_seed, uint32_t *n_distance, uint32_t *n_beyond, uint32_t *n_undecided,
                         uint32_t *n_realigned, uint64_t *distance_cells, float *ms_distance, float *ms_pick);

/* The pair-aware pick: reads that come as PAIRS (two mates sequenced from the two ends of one fragment, on opposite strands)
 * are placed together.  A call of its own, like bmv_annotate and bmv_clip: it needs no reads and no genome, only numbers per
 * alignment -- the views' text_start, text_len, text_rc and query_len, edits and end as bmv_best returns them (BMV_BEYOND: not
 * known), and contig, the reference sequence an alignment lies on (NULL: all on one).  Groups as in bmv_align_best; the mates of
 * pair p are the groups 2p and 2p + 1.  All coordinates are signed 64-bit, in the concatenated genome:
 *   known(a)            edits[a] != BMV_BEYOND
 *   text_rc[a] == 0     R(a) = text_start + end (exact), L(a) = R(a) - query_len (an estimate: only the end is exact)
 *   text_rc[a] != 0     L(a) = text_start + text_len - end (exact), R(a) = L(a) + query_len (the estimate)
 *   locus(a)            (text_rc != 0, R forward / L reverse): the coordinate host/best_mapq.h tells loci apart by
 *   own winner of g     the lowest known index of the group with the smallest edits; BMV_BEYOND when there is none
 *   proper (i, j)       i in group 2p, j in group 2p + 1, both known, on one contig, on different strands, and with f the forward
 *                       and r the reverse one: L(f) <= L(r), R(f) <= R(r), min_frag <= R(r) - L(f) <= max_frag
 *   the pick of p       the proper combination that minimises (edits[i] + edits[j], i, j) lexicographically, the sum in 64 bits
 *   s1, s2              the pick's sum; the smallest sum over the proper combinations (i', j') with locus(i') != locus(i) or
 *                       locus(j') != locus(j)
 * Outputs (bmv_pairs; any pointer may be NULL): out_pick[g] the picked alignment of group g -- the group's own winner when the
 * pair has no proper combination --, out_proper[p] 0 or 1, out_s1[p] and out_s2[p] (BMV_PAIR_NONE where undefined),
 * out_winner[g] the own winner.
 * Checks: group_offset as in bmv_align_best; n_groups even; min_frag <= max_frag; text_start below 2^62: BMV_ERR_ARG, nothing
 * ran and the context stays usable.  The call leaves untouched what every other result call returns.
 * How (bmv_pair.hip.h): a wave per pair; up to 64 candidates of the second mate in the lanes, the first mate's walked
 * wave-uniformly, both dimensions looped; the pick and s2 are minima taken across the wave. */
#define BMV_PAIR_NONE UINT64_MAX
int  bmv_pair(bmv_ctx *ctx, const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len,
              const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
              uint32_t n_groups, uint32_t min_frag, uint32_t max_frag);
/* Of the last bmv_pair or bmv_align_paired: out_pick and out_winner n_groups entries, the others n_groups / 2. */
int  bmv_pairs(bmv_ctx *ctx, uint32_t *out_pick, uint8_t *out_proper, uint64_t *out_s1, uint64_t *out_s2, uint32_t *out_winner);
/* Of the last bmv_pair or bmv_align_paired: the pair kernel's time in ms and the combinations it examined (the sum over the
 * pairs of the product of the two group sizes). */
int  bmv_last_pair_stats(bmv_ctx *ctx, float *ms_pair, uint64_t *n_combinations);

/* bmv_align_best for pairs: the same batch and groups (n_groups even), plus contig, min_frag and max_frag as bmv_pair takes them.
 * Four rounds: bmv_align_best's seed and distance rounds; its restriction of (d, end) to d <= best + margin, which makes what
 * follows independent of hint; the bmv_pair kernel on those arrays where they lie on the device; the full alignment of every
 * pick that has none yet.  bmv_results: the PICKS carry exactly bmv_align_long's score, begin and CIGAR, everything else score
 * BMV_REJECTED, begin 0 and no entries; bmv_best returns what it returns after bmv_align_best (out_winner: the own winners);
 * bmv_pairs the pair outputs; bmv_last_best_stats as after bmv_align_best, n_realigned counting the picks aligned in the last
 * round.  Checks are bmv_align_best's and bmv_pair's. */
int  bmv_align_paired(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                      const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                      uint32_t n, const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                      const uint32_t *contig, uint32_t min_frag, uint32_t max_frag, uint64_t *total_cigar);

/* The fragment spans: what a batch of pairs says about the range a proper pair may span, so that the range can be learned from
 * the data instead of being typed.  A call of its own over numbers alone, like bmv_pair, with bmv_pair's arguments; known, L, R,
 * locus, own winner and proper are bmv_pair's, word for word.  Integers only:
 *   settled(g)          group g has an own winner w and every known alignment of the group has locus == locus(w).  (Overlapping
 *                       windows of neighbouring buckets find one alignment twice; that does not unsettle a group.  Over the
 *                       alignments within best + margin -- what bmv_paired_begin looks at -- settled is exactly "best_mapq
 *                       would say 60".)
 *   span[p]             with w1, w2 the own winners of the groups 2p and 2p + 1: R(r) - L(f) when both groups are settled and
 *                       proper(w1, w2) holds under min_frag = 1, max_frag = cap; else 0, the pair is uninformative
 *   hist[s]             for 0 <= s <= cap the number of pairs with span == s; hist[0] counts the uninformative pairs and the
 *                       sum over hist is n_groups / 2
 * The range itself is the host's (bm::frag_range, host/frag_range.h; verify.frag_range), from one histogram or from the sum of
 * several: n = the sum of hist[s] over s >= 1; learned iff n >= max(1, min_pairs), else the caller's fallback range unchanged;
 * with v the informative spans in ascending order, Qk = v[floor(k n / 4)] for k = 1, 2, 3, IQR = Q3 - Q1,
 * slack = max(3 IQR, ceil(Q2 / 4)), min_frag = max(1, Q1 - slack) in signed arithmetic, max_frag = Q3 + slack.  A definition by
 * choice, like the MAPQ scales.
 * Checks: bmv_pair's, and 1 <= cap <= 65 535: BMV_ERR_ARG, nothing ran and the context stays usable.  The call leaves untouched
 * what every other result or stats call returns -- those of bmv_annotate, bmv_clip, bmv_realign, bmv_leftalign, bmv_split,
 * bmv_split_pick and bmv_rescue too -- and a pending bmv_paired_begin stays pending.
 * How (bmv_frag.hip.h): the span kernel is a wave per pair -- the two own winners, then the settled test as a walk over either
 * group in lane chunks of 64 with a ballot each --; the histogram kernel strides a resident grid over span[], the bins private
 * to a block in LDS while cap + 1 <= 16 384 and only the non-zero ones flushed by global atomic adds, beyond that global atomic
 * adds, one per distinct span among a wave's 64.  The call zeroes the device bins itself, every time. */
int  bmv_frag_spans(bmv_ctx *ctx, const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc,
                    const uint32_t *query_len, const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t n,
                    const uint32_t *group_offset, uint32_t n_groups, uint32_t cap);
/* Of the last bmv_frag_spans or bmv_paired_begin with cap > 0: out_span n_groups / 2 entries, out_hist cap + 1; either may be
 * NULL. */
int  bmv_frag(bmv_ctx *ctx, uint32_t *out_span, uint64_t *out_hist);
/* Of the same: the two kernels' time in ms and the informative pairs, the sum of hist[s] over s >= 1. */
int  bmv_last_frag_stats(bmv_ctx *ctx, float *ms_kernels, uint32_t *n_informative);

/* bmv_align_paired in two halves, so that the range can be settled between them -- from the spans of this context and of every
 * other context that holds a share of the same block of reads.  bmv_align_paired itself is begin(cap = 0) + finish.
 * bmv_paired_begin: bmv_align_paired's arguments without the range, its checks except the range's, plus cap: 0, or as
 * bmv_frag_spans checks it.  Runs bmv_align_best's seed and distance rounds and the restriction; for cap > 0 the two
 * bmv_frag_spans kernels on the restricted (edits, end) where they lie on the device, which fills bmv_frag's row (cap = 0 leaves
 * that row as it is).  The arrays passed in must stay valid and unchanged until bmv_paired_finish returns: the picks are aligned
 * from them.  Until then the bmv_results row is unspecified.
 * bmv_paired_finish: the pair kernel under [min_frag, max_frag], the full alignment of every pick that has none yet, the
 * results.  After it bmv_results, bmv_best, bmv_pairs, bmv_last_best_stats, bmv_last_pair_stats and bmv_last_stats return
 * exactly what bmv_align_paired with that range returns for the batch (bmv_last_stats' ms includes the frag kernels').
 * min_frag > max_frag: BMV_ERR_ARG, and the begin stays pending -- a corrected call may follow.  BMV_ERR_STATE, nothing ran and
 * the context stays usable, when no successful begin is pending: none was made, finish ran already (also one that failed later
 * than its checks), or another call that aligns came in between -- bmv_align, bmv_align_long, bmv_align_bounded, bmv_align_best,
 * bmv_align_paired, a new bmv_paired_begin that failed (the two end a pending begin even when their own checks refuse
 * them: the one exception to "a refused call changes nothing"), and bmv_rescue when it falls back to the aligner.  bmv_frag_spans,
 * bmv_frag, bmv_pair and every result accessor may come in between.  So may bmv_annotate, bmv_clip, bmv_realign, bmv_leftalign,
 * bmv_split, bmv_split_pick and a bmv_rescue none of whose queries has more than 512 bases: they neither end the begin nor
 * write where it left its arrays.  Whatever came in between, and however large its batch was, the finish returns what
 * bmv_align_paired returns for the begin's batch. */
int  bmv_paired_begin(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                      const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                      uint32_t n, const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                      const uint32_t *contig, uint32_t cap);
int  bmv_paired_finish(bmv_ctx *ctx, uint32_t min_frag, uint32_t max_frag, uint64_t *total_cigar);

/* Mate rescue: a mate without a usable candidate (a repeat whose bucket list was cleared, k-mers that failed the quality filter,
 * a wrong bucket) is sought beside a known alignment of its partner.  A call of its own, like bmv_pair, bmv_annotate and
 * bmv_clip.  A batch holds n JOBS; job j places one mate, the query reads[query_start[j], +query_len[j]), beside an ANCHOR: a
 * known alignment of its partner given as bmv_pair takes one -- the view anchor_text_start / anchor_text_len / anchor_text_rc,
 * anchor_query_len and anchor_end -- on the contig [contig_start[j], contig_end[j]) of the concatenated genome.
 * The window is derived on the device in signed 64-bit genome coordinates.  L, R and proper are exactly bmv_pair's; La, Ra are
 * the anchor's by bmv_pair's two formulas.  With m = query_len[j], k = min(max_edits[j], m) and [c0, c1) the contig:
 *   anchor forward      the mate is sought on the reverse strand (out_text_rc = 1); its admissible LEFT end is x in [x_lo, x_hi],
 *                       x_lo = max(La, Ra - m, La + min_frag - m), x_hi = La + max_frag - m;
 *                       the view is [ws, we), ws = max(c0, x_lo), we = min(c1, x_hi + m + k)
 *   anchor reverse      the mate is sought forward (out_text_rc = 0); its admissible RIGHT end is z in [z_lo, z_hi],
 *                       z_lo = Ra + m - max_frag, z_hi = min(La + m, Ra, Ra + m - min_frag);
 *                       ws = max(c0, z_lo - m - k), we = min(c1, z_hi)
 *   out_text_start = ws, out_text_len = max(0, we - ws)
 * The far border of the view, as the aligner walks it, is the last admissible end, and there is room for m + k columns before
 * the first admissible one: every alignment within k edits that ends admissibly lies inside the view, unless the contig cuts
 * it, and there the cut is right.
 * The result is exact and states no heuristic.  With (score, begin, CIGAR) what bmv_align_long returns for the query against
 * the view, d = -score and end = begin + R (tie rule (1)): out_edits[j] = d and out_end[j] = end when d <= k, else BMV_BEYOND
 * and 0; an empty view, m = 0 and a view shorter than m - k are all BMV_BEYOND.  out_proper[j] is bmv_pair's proper(anchor,
 * rescued) evaluated on the rescued view and out_end, 0 when beyond.  A best placement that ends before the first admissible
 * end is reported with its distance and proper = 0; the caller does not use it.
 * Checks before anything runs (BMV_ERR_ARG, the message names the job, the context stays usable): min_frag <= max_frag;
 * contig_start <= contig_end <= the genome's length; anchor_end <= anchor_text_len; the anchor's view inside the genome and
 * anchor_text_start below 2^62; the query inside `reads`; max_frag + k below 2^32 (what a view may hold).  n = 0 is fine.  The
 * call leaves untouched what bmv_results, bmv_best, bmv_pairs, bmv_annotations, bmv_clipped and their stats calls return.
 * How (bmv_rescue.hip.h): a plan kernel writes the views; the distance kernel keeps every word of a query of up to 512 bases in
 * one lane and runs the plain recurrence over the whole view (row 0 is free and the placement unknown: there is no band to
 * keep), watching row m for a score <= k; a job is cut along the text into `parts` (a power of two, 1 .. 64) in neighbouring
 * lanes, part p walking from max(0, b_p - m - k) with b_p = floor(p n / parts) and counting end columns in (b_p, b_{p+1}] --
 * exact, because an alignment within k edits that ends at e begins at or after e - m - k -- and the parts' minima meet by
 * shuffles, the later column winning a tie; a finish kernel applies the rule.  The host picks `parts` per call from the job
 * count and the device's resident lanes, no part shorter than its warm-up (BMV_RESCUE_PARTS=<n> forces it: tests,
 * experiments).  A query of more than 512 bases is aligned in full on its planned view: time, never a refusal. */
int  bmv_rescue(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *anchor_text_start,
                const uint32_t *anchor_text_len, const uint8_t *anchor_text_rc, const uint32_t *anchor_query_len,
                const uint32_t *anchor_end, const uint64_t *contig_start, const uint64_t *contig_end, const uint64_t *query_start,
                const uint32_t *query_len, const uint32_t *max_edits, uint32_t n, uint32_t min_frag, uint32_t max_frag);
/* Of the last bmv_rescue: n entries each; any pointer may be NULL. */
int  bmv_rescued(bmv_ctx *ctx, uint64_t *out_text_start, uint32_t *out_text_len, uint8_t *out_text_rc, uint32_t *out_edits,
                 uint32_t *out_end, uint8_t *out_proper);
/* Of the last bmv_rescue: the kernels' time in ms (plan, distance, finish, and the aligner's for queries beyond 512 bases), 64 x
 * the (64-row word, text column) steps of the distance kernel -- warm-up columns included -- plus query_len x text_len of what
 * the aligner took, and the parts a job was cut into.  Any pointer may be NULL. */
int  bmv_last_rescue_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_cells, uint32_t *parts);

/* Who owns what.  Every result accessor and every bmv_last_*_stats returns what ITS OWN last successful call left, whatever
 * other calls the context has served since, however large their batches were:
 *   bmv_results, bmv_last_stats          bmv_align, bmv_align_long, bmv_align_bounded, bmv_align_best, bmv_align_paired, and
 *                                        bmv_paired_begin + bmv_paired_finish, which count as bmv_align_paired in every row
 *   bmv_last_bounded_stats               bmv_align_bounded alone: bmv_align_best and bmv_align_paired use the screen's recurrence
 *                                        in kernels and counters of their own and leave it untouched, as do bmv_align and
 *                                        bmv_align_long
 *   bmv_best, bmv_last_best_stats        bmv_align_best, bmv_align_paired; after a plain bmv_align, bmv_align_long or
 *                                        bmv_align_bounded they still return what the last of those two left (nothing, and
 *                                        zeros, on a context that never made one)
 *   bmv_pairs, bmv_last_pair_stats       bmv_pair, bmv_align_paired, bmv_paired_finish
 *   bmv_frag, bmv_last_frag_stats        bmv_frag_spans, bmv_paired_begin with cap > 0
 *   bmv_rescued, bmv_last_rescue_stats   bmv_rescue; its fallback for queries beyond 512 bases runs bmv_align_long's kernels and
 *                                        puts bmv_results and bmv_last_stats back as it found them
 *   bmv_segments, bmv_last_split_stats   bmv_split, bmv_split_pick
 *   bmv_annotations, bmv_clipped, bmv_realigned, bmv_leftaligned and their stats: the one call each is named after
 *   bmv_overlapped, bmv_last_overlap_stats   bmv_overlap
 * A call changes nothing outside its row.  n = 0 is a successful call: it leaves empty results and zero counts in its row.  A
 * call refused by its checks before anything runs -- every BMV_ERR_ARG, and BMV_ERR_UNSUPPORTED from bmv_align_long,
 * bmv_realign and bmv_leftalign -- changes nothing at all.  One refusal comes later: bmv_align_bounded, bmv_align_best and
 * bmv_align_paired hand sub-batches to bmv_align_long, and when an alignment's trace does not fit the scratch there
 * (BMV_ERR_UNSUPPORTED) the call's own row is unspecified until the next successful call of that row; every other row stays.
 *
 * Results of the last bmv_align, bmv_align_long, bmv_align_bounded, bmv_align_best or bmv_align_paired:
 *   out_score[a]        alignment.score() = -(edit distance)                       (bucket_locator.h:570)
 *   out_begin[a]        alignment.sequence1_begin_position(), 0-based in the text  (:576)
 *   out_cigar_offset    n + 1 entries; alignment a owns out_cigar[offset[a] .. offset[a+1])
 *   out_cigar           total_cigar packed entries, in alignment order, 5' to 3' of the query */
int  bmv_results(bmv_ctx *ctx, int32_t *out_score, uint32_t *out_begin, uint64_t *out_cigar_offset,
                 uint32_t *out_cigar);

/* Kernel time of the last bmv_align (or bmv_align_long) in ms (edit-distance columns + traceback, all chunks) and the number
 * of dynamic-programming cells it stands for (sum of query_len * text_len).  After bmv_align_bounded, bmv_align_best and
 * bmv_align_paired: the whole call's kernel time, and the cells of the WHOLE batch -- the sum over every alignment handed in,
 * also the ones rejected, beyond the margin or never aligned in full. */
int  bmv_last_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_cells);

/* The annotation pass: what a SAM record needs beyond score, begin and an M/I/D CIGAR, for alignments whose CIGARs are known.
 * A call of its own: it does not care which of bmv_align, bmv_align_long or bmv_align_bounded produced the CIGARs (or whether a
 * caller wrote them by hand), and it leaves what bmv_results, bmv_last_stats and bmv_last_bounded_stats return untouched.
 * Input per alignment a: the views bmv_align takes, plus begin[a] and the entries cigar[cigar_offset[a] .. cigar_offset[a+1])
 * as bmv_results returns them -- M/I/D, 5' to 3' of the query, begin counted in the text as the aligner saw it (in the reverse
 * complement when text_rc[a] != 0).  Output per alignment, in FORWARD-strand coordinates, with R = sum of the M and D lengths:
 *   out_pos[a]          begin when text_rc == 0, else text_len - begin - R: 0-based in the forward window
 *   out_ref_len[a]      R
 *   out_xcigar          every M run split into maximal runs of equal (BMV_OP_EQ) and unequal (BMV_OP_X) bases, I and D as they
 *                       are; equality is on dna4 ranks on both sides (N and IUPAC fold, either case), the comparison the aligner
 *                       scored with; for text_rc != 0 the entries come in reversed order, so that they read along the forward
 *                       strand; adjacent entries never share an op.  out_xcigar_offset: n + 1 entries
 *   out_nm[a]           sum of the X, I and D lengths (= -score for a CIGAR that came from the aligner)
 *   out_ref_bases       the forward-strand reference base under every X and D column, in forward order, one folded letter
 *                       (A C G T) each -- for text_rc != 0 the complement of what the aligner compared against; the payload of
 *                       SAM's MD tag, whose text is formatted on the host.  out_ref_offset: n + 1 entries
 * An empty CIGAR (an alignment bmv_align_bounded rejected, a zero-length query) gives nm = pos = ref_len = 0 and no entries.
 * The batch is checked on the host before anything is launched: views inside `reads` and the genome, every op M, I or D, every
 * length > 0, adjacent entries of different ops, M + I lengths = query_len, begin + R <= text_len, fewer than 2^32 - query_len
 * entries per alignment.  A failure returns BMV_ERR_ARG, the message names the alignment, nothing ran and the context stays
 * usable.  Any lengths that fit uint32 (entry lengths: 28 bits); no scratch beyond the inputs and outputs.
 * How: a wave per alignment walks text and query once in forward-strand order, 64 columns a step (bmv_annotate.hip.h); sizes are
 * counted first, two prefix sums place the packed outputs, a second walk writes them. */
int  bmv_annotate(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                  const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                  const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n,
                  uint64_t *total_xcigar, uint64_t *total_ref_bases);
/* Results of the last bmv_annotate; any pointer may be NULL. */
int  bmv_annotations(bmv_ctx *ctx, uint32_t *out_nm, uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset,
                     uint32_t *out_xcigar, uint64_t *out_ref_offset, uint8_t *out_ref_bases);
/* Kernel time of the last bmv_annotate in ms (count pass, prefix sums, write pass) and the alignment columns it walked (sum of
 * all CIGAR entry lengths). */
int  bmv_last_annotate_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_columns);

/* The clipping pass: bmv_annotate's record with low-identity ends soft-clipped.  The aligners align the WHOLE query (unit
 * costs: free end gaps in the query would make clipping everything optimal), so a read that overhangs its window, carries an
 * adapter or has a chimeric or low-quality end gets those bases spread over X, I and D columns at an end of its alignment.  This
 * post-pass over the edit path keeps the best-scoring contiguous stretch of alignment columns and reports the rest as S.
 * A call of its own, the sibling of bmv_annotate: the same inputs (CIGARs M/I/D from any of the three align calls or written by
 * hand), the same checks on the host before anything is launched (BMV_ERR_ARG, the message names the alignment, nothing ran, the
 * context stays usable), plus 1 <= match, penalty <= 1024 (else BMV_ERR_ARG).  It leaves untouched what bmv_results,
 * bmv_annotations, bmv_last_stats, bmv_last_bounded_stats and bmv_last_annotate_stats return.
 * Semantics.  Take alignment a's columns in FORWARD-strand order, the order bmv_annotate emits its entries in: 0 .. C-1.  Column
 * i weighs w(i) = +match when it is an = column, -penalty when it is an X, I or D column (equality on dna4 ranks, as in
 * bmv_annotate).  P[0] = 0, P[i+1] = P[i] + w(i), in signed 64-bit arithmetic.  The kept range [l, r) maximises P[r] - P[l] over
 * 0 <= l <= r <= C; among the maximisers it has the smallest r, then the largest l.  So a non-empty range begins and ends on an
 * = column, and an alignment without any = column keeps the empty range l = r = 0.  Output per alignment:
 *   out_score[a]        P[r] - P[l]
 *   out_clip_left[a]    the query-consuming columns (=, X, I) before l;  out_clip_right[a]: those from r on
 *   out_pos[a]          bmv_annotate's pos plus the reference-consuming columns (=, X, D) before l
 *   out_ref_len[a]      the reference-consuming columns inside [l, r)
 *   out_nm[a]           the X, I and D columns inside [l, r)
 *   out_xcigar          an S entry (BMV_OP_S) of clip_left when that is > 0; bmv_annotate's = / X / I / D entries restricted to
 *                       [l, r), an entry the range cuts through shortened; an S entry of clip_right when that is > 0.  Adjacent
 *                       entries never share an op.  out_xcigar_offset: n + 1 entries
 *   out_ref_bases       the forward-strand reference letter under the kept X and D columns.  out_ref_offset: n + 1 entries
 * Always: clip_left + the kept =, X and I lengths + clip_right = query_len, and pos + ref_len <= text_len.
 * An empty range with query_len > 0 gives one S entry of query_len (clip_left 0, clip_right query_len) and pos = ref_len = nm =
 * score = 0.  An empty CIGAR gives no entries and zeros everywhere, as in bmv_annotate.
 * How: a wave per alignment and bmv_annotate's walk, three times (bmv_clip.hip.h): the range pass finds [l, r) with a prefix
 * minimum and a maximum across the wave per 64 columns, then sizes are counted, two prefix sums place the packed outputs, and a
 * last walk writes them.  No scratch beyond the inputs and outputs. */
int  bmv_clip(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
              const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
              const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t penalty,
              uint64_t *total_xcigar, uint64_t *total_ref_bases);
/* Results of the last bmv_clip; any pointer may be NULL. */
int  bmv_clipped(bmv_ctx *ctx, int64_t *out_score, uint32_t *out_clip_left, uint32_t *out_clip_right, uint32_t *out_nm,
                 uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset, uint32_t *out_xcigar,
                 uint64_t *out_ref_offset, uint8_t *out_ref_bases);
/* Kernel time of the last bmv_clip in ms (range pass, count pass, prefix sums, write pass) and the alignment columns it walked
 * (sum of all CIGAR entry lengths). */
int  bmv_last_clip_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_columns);

/* The overlap pass: bmv_clip's record for the two mates of a pair, soft-clipped at one cut so that no reference base lies under
 * both.  In short-insert libraries most proper pairs overlap, and everything that counts bases per reference position (depth,
 * pileup, genotypes) sees the fragment twice there; this is what fgbio ClipBam --clip-overlapping-reads and bamUtil clipOverlap
 * do to a finished BAM, done where both mates and their edit paths are at hand.  A call of its own, of the bmv_annotate /
 * bmv_clip family.
 * Inputs: bmv_clip's (the views, begin, M/I/D entries 5' to 3' of the query, match, penalty) plus
 *   mate[a]             the batch index of alignment a's mate, or BMV_NO_MATE
 *   contig[a]           as bmv_pair takes it; NULL: all on one contig
 * Mode.  match == 0 && penalty == 0 means "no score clipping": the base range of every alignment is all its columns [0, C) and
 * out_score is 0.  Otherwise 1 <= match, penalty <= 1024 and the base range [l, r) is exactly bmv_clip's.
 * Coordinates.  Columns are in FORWARD-strand order, as bmv_annotate emits them.  g(i) = text_start[a] + (bmv_annotate's pos) +
 * (the reference-consuming columns before i), in signed 64-bit arithmetic, in the concatenated genome; G0 = g(l), G1 = g(r).
 * Which pairs are cut.  A pair (a, b = mate[a]) is cut only if all of these hold, otherwise both mates come back exactly as the
 * base pass gives them:
 *   both base ranges are non-empty;  contig[a] == contig[b];
 *   with `first` the mate of smaller (G0, index) and `second` the other: G1(first) <= G1(second);
 *   o = G1(first) - G0(second) > 0;
 *   both columns named under "kept ranges" exist.
 * Containment (G1(first) > G1(second)), disjoint spans, different contigs and an empty range are all "not cut".  Strands are not
 * looked at.
 * The cut.  m = G0(second) + floor(o / 2).
 * Kept ranges.  `first` keeps [l, r'): r' - 1 is the last M column (= or X, not I or D) of [l, r) with g < m.  `second` keeps
 * [l', r): l' is the first M column of [l, r) with g >= m.  So the kept ranges never begin or end on I or D at the cut, no
 * reference position lies under both, and G0(first) and G1(second) do not move.
 * Output per alignment: bmv_clipped's layout, value for value, for the final range -- out_clip_left, out_clip_right, out_pos,
 * out_ref_len, out_nm, out_xcigar with S entries, out_ref_bases and the offsets -- with
 *   out_score[a]        match x (the = columns kept) - penalty x (the X, I and D columns kept)
 *   out_cut[a]          the query bases the cut added to the soft clips; 0 for an untouched alignment
 * Two identities follow.  With mate[a] == BMV_NO_MATE everywhere and match > 0 the outputs are bmv_clipped's, byte for byte.  With
 * match == penalty == 0 (and no mates) they are bmv_annotations' (no S entries, clips 0).
 * LEFT OUT: merging the two mates' base qualities where they agree; hard clips; any tag that records the cut; containment and
 * dovetail pairs; an insertion exactly at the cut, which is clipped in BOTH mates (its columns carry g = m in the first and lie
 * before l' in the second), so its bases are seen in neither.
 * Checks on the host before anything is launched: bmv_clip's, plus: the scores are (0, 0) or in range; mate[a] < n or
 * BMV_NO_MATE; mate[a] != a; mate[mate[a]] == a; text_start below 2^62.  BMV_ERR_ARG, the message names the alignment, nothing
 * ran and the context stays usable.  n = 0 succeeds.  The call leaves untouched what every other result or stats call returns,
 * and a pending bmv_paired_begin stays pending.
 * How (bmv_overlap.hip.h): a wave per alignment and bmv_annotate's walk; the two mates meet between launches, no kernel waits
 * for another workgroup.  bmv_clip's range pass (or nothing) gives l, r; a span pass G0, G1; a pass per alignment reads both mates'
 * spans and decides m; a pass restricts the range -- l' and r' depend on the CIGAR entries alone, every M column being = or X --;
 * then bmv_clip's count pass, two prefix sums and its write pass run on the final range. */
#define BMV_NO_MATE UINT32_MAX
int  bmv_overlap(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                 const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *mate, const uint32_t *contig, uint32_t n,
                 uint32_t match, uint32_t penalty, uint64_t *total_xcigar, uint64_t *total_ref_bases);
/* Results of the last bmv_overlap; any pointer may be NULL. */
int  bmv_overlapped(bmv_ctx *ctx, int64_t *out_score, uint32_t *out_clip_left, uint32_t *out_clip_right, uint32_t *out_nm,
                    uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset, uint32_t *out_xcigar,
                    uint64_t *out_ref_offset, uint8_t *out_ref_bases, uint32_t *out_cut);
/* Of the last bmv_overlap: the kernels' time in ms (every pass and the prefix sums), the alignment columns it walked (sum of all
 * CIGAR entry lengths), the pairs cut and the sum of out_cut.  Any pointer may be NULL. */
int  bmv_last_overlap_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_columns, uint64_t *pairs_cut, uint64_t *bases_cut);

/* The realignment pass: an affine-gap alignment beside a known edit path.  Everything the aligners return comes from unit
 * costs, under which a 6-base deletion and six scattered 1-base gaps cost the same, so the traceback's tie rules decide where
 * indels fall; consumers of SAM assume gap-affine alignments and an AS:i on a match / mismatch / gap-open / gap-extend scale.
 * A full Gotoh matrix is out of the question, but the affine optimum lies near the edit path we hold: this post-pass runs the
 * recurrence in a band of at most 64 columns that follows that path.  A call of its own, of the bmv_annotate / bmv_clip family:
 * the same inputs (the views, begin, M/I/D entries 5' to 3' of the query, begin counted in the text as the aligner saw it) and
 * the same checks on the host before anything is launched (BMV_ERR_ARG, the message names the alignment, nothing ran, the
 * context stays usable); in addition 1 <= match, mismatch, gap_open, gap_extend <= 1024 and 1 <= band <= 31, else BMV_ERR_ARG;
 * and, so that the kernel can work in 32 bits, per alignment with a non-empty CIGAR
 *   (query_len + text_len) * max(match, mismatch, gap_extend) + gap_open < 2^30, and
 *   the given path's own worst case -- max(match, mismatch) per M column, gap_open + L gap_extend per I or D entry of length L --
 *   + gap_open + (query_len + text_len) * gap_extend < 2^30 (it bounds every cell of the band from below),
 * else BMV_ERR_UNSUPPORTED, the message names the alignment.  The call leaves untouched what every other result or stats call
 * returns.  The output (bmv_realigned) has the shape of bmv_results, so it can be handed straight to bmv_annotate or bmv_clip.
 * The contract is exact and stated on the outputs only.  m = query_len, n = text_len, w = band; T is the text as the aligner
 * saw it (reverse-complemented for text_rc != 0); equality is on dna4 ranks on both sides, as in bmv_annotate; cells are (i, j),
 * 0 <= i <= m, 0 <= j <= n.
 *   the given path     starts at (0, begin); an M column moves (+1, +1), I moves (+1, 0), D moves (0, +1).  p(i) is the first
 *                      column the path visits in row i, q(i) the last
 *   the band           row i holds the columns [max(0, p(i) - w), min(n, q(i) + w)]; everything else is absent.  An absent
 *                      operand never wins a maximum; a cell all of whose operands are absent is absent
 *   pass-through       if any row has q(i) - p(i) > 63 - 2w -- a D entry longer than 63 - 2w -- the alignment is not realigned,
 *                      and neither is one with an empty CIGAR: out_realigned = 0, begin and the entries are returned as given,
 *                      out_score is the affine score of the given path: +match per equal M column, -mismatch per unequal one,
 *                      -(gap_open + L gap_extend) per I or D entry of length L (an empty CIGAR: score 0, no entries).
 *                      Otherwise every row's band is at most 64 columns and out_realigned = 1
 *   recurrence         s(i, j) = +match if query[i - 1] equals T[j - 1], else -mismatch  (i >= 1)
 *                      H(0, j) = 0 on row 0's band; Ins(0, .) and Del(0, .) are absent
 *                      Ins(i, j) = max(H(i - 1, j) - gap_open - gap_extend, Ins(i - 1, j) - gap_extend)
 *                      Del(i, j) = max(H(i, j - 1) - gap_open - gap_extend, Del(i, j - 1) - gap_extend)
 *                      H(i, j)   = max(H(i - 1, j - 1) + s(i, j), Ins(i, j), Del(i, j))
 *   out_score          the maximum of H(m, j) over row m's band; the alignment ends at the LAST column that attains it (tie
 *                      rule (1) above).  The given path lies inside the band, so out_score >= the given path's affine score
 *   traceback          in H the order is diagonal, then Ins, then Del (tie rule (2)); in Ins and in Del a tie goes to "open",
 *                      the shorter gap.  The walk stops when it reaches row 0 in state H; that column is out_begin.  Entries
 *                      are M / I / D, 5' to 3' of the query, adjacent entries never share an op; a result never begins or ends
 *                      with D
 * Under these rules gaps in a repeat are pushed towards the START of the text AS THE ALIGNER SAW IT -- for text_rc != 0 that is
 * the right end on the forward strand.  bmv_leftalign (below) normalises them on the forward strand.
 * The scores are a choice of the caller (the tool's default 1, 4, 6, 1 is the common short-read scale, not a measurement).
 * How (bmv_realign.hip.h): a wave per alignment, a lane per band column, the wave stepping row by row along the CIGAR; the Del
 * chain of a row by a prefix maximum across the lanes; a byte of direction codes per cell to the scratch, the batch taken in
 * pieces that fit it (BMV_SCRATCH_MB applies; an alignment whose codes alone do not fit fails the call with
 * BMV_ERR_UNSUPPORTED before anything runs); the traceback walks the codes 64 rows at a time out of LDS. */
int  bmv_realign(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                 const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t mismatch,
                 uint32_t gap_open, uint32_t gap_extend, uint32_t band, uint64_t *total_cigar);
/* Results of the last bmv_realign: n entries each, out_cigar_offset n + 1, out_cigar total_cigar; any pointer may be NULL. */
int  bmv_realigned(bmv_ctx *ctx, int32_t *out_score, uint32_t *out_begin, uint8_t *out_realigned, uint64_t *out_cigar_offset,
                   uint32_t *out_cigar);
/* Of the last bmv_realign: the kernels' time in ms (forward, traceback, scan and gather, all pieces), 64 x the query rows of
 * the realigned alignments (the lanes a wave steps through, whatever the band), and the alignments passed through.  Any
 * pointer may be NULL. */
int  bmv_last_realign_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_cells, uint32_t *n_passed_through);

/* The normalisation pass: every I and D entry of a known M/I/D path moved to its leftmost equivalent place ON THE FORWARD
 * STRAND.  The aligners' tie rules, and bmv_realign's, push an indel that lies in a repeat (a homopolymer, a microsatellite,
 * a tandem copy) towards the start of the text as the aligner saw it -- for a reverse-strand read the right end of the run on
 * the forward strand --, so forward and reverse reads write the same event at two coordinates; every consumer of SAM assumes
 * the leftmost one.  A call of its own, of the bmv_annotate / bmv_clip / bmv_realign family: bmv_annotate's inputs and its
 * checks on the host before anything is launched (BMV_ERR_ARG, the message names the alignment, nothing ran, the context stays
 * usable); in addition BMV_ERR_UNSUPPORTED, the message naming the alignment and nothing having run, when one alignment's I
 * lengths or its D lengths (or its M lengths: M entries merge too) sum to 2^28 or more -- a merged entry would not fit 28
 * bits --, or when one alignment's stack alone (4 bytes per entry and 4 more per gap entry) does not fit the scratch
 * (BMV_SCRATCH_MB).  The call leaves untouched what every other result or stats call returns.  The output (bmv_leftaligned)
 * has the shape of bmv_results / bmv_realigned -- begin and M/I/D entries in the aligner's orientation --, so it can be handed
 * straight to bmv_annotate or bmv_clip.  The contract is exact and stated on the outputs only.
 *   the forward view   of alignment a: W is the window as it lies in the genome; pos is bmv_annotate's pos; Qf is the query
 *                      read along the forward strand (for text_rc != 0 its reverse complement); the entries are taken in
 *                      forward order (for text_rc != 0 reversed).  Equality is on dna4 ranks on both sides, as in bmv_annotate;
 *                      two complemented bases are equal exactly when the originals are, so nothing has to be complemented
 *   the walk           through the entries left to right, the output kept as a stack, with a reference cursor p (from pos) and
 *                      a query cursor q (from 0).  An M entry is appended (it merges with an M on top of the stack) and moves
 *                      both cursors.  A gap entry of op g and length L begins at (p, q) and carries a count pend = 0 of the M
 *                      columns it has passed.  For the gap, repeat:
 *                        (1) the stack is empty: a D is dropped (pos += L, dropped += L), an I is pushed.  Stop.
 *                        (2) the top is M of length k: s is the largest value <= k such that for every t = 1..s
 *                            W[p - t] == W[p - t + L] (a D) / Qf[q - t] == Qf[q - t + L] (an I).  p -= s, q -= s, pend += s, the M
 *                            becomes k - s.  If s < k, push the gap and stop; otherwise pop the emptied M and repeat.
 *                        (3) the top is a gap of the same op and length L': pop it, L += L', p -= L' (a D) / q -= L' (an I),
 *                            one merge is counted.  Repeat: the merged gap goes on moving under its new length.
 *                        (4) the top is a gap of the other op: push the gap and stop.
 *                      After the gap stops, an M of pend is appended (it merges with a following M) and the cursors stand
 *                      behind the gap as given.  At the end of the walk a D on top of the stack is dropped, its length added
 *                      to dropped.
 *   what follows       each step swaps an M column for one of the same =/X status, so NM and any affine score change only
 *                      through merges and drops: nm_out = nm_in - dropped; M + I lengths = query_len; pos' + R' <= text_len;
 *                      adjacent entries never share an op; the result never begins or ends with D; it has at most E + (gap
 *                      entries) entries; the pass is idempotent
 *   out_begin          in the aligner's orientation: pos' for text_rc == 0, else text_len - pos' - R' (R' the M and D lengths
 *                      of the result)
 *   out_cigar          entries 5' to 3' of the query, at out_cigar_offset (n + 1)
 *   out_changed        1 when a gap moved or bases were dropped -- exactly when begin or the entries differ from those given
 *   out_dropped        the D bases dropped at the two ends
 *   an empty CIGAR     begin as given, no entries, zeros
 * How (bmv_leftalign.hip.h): a wave per alignment walks the entries in uniform registers, 64 fetched at a time; for a gap lane
 * t - 1 compares the two bytes of shift t, one ballot and a count of trailing ones give up to 64 columns of shift a step; the
 * stack's body lies in a slot of the scratch, the batch taken in pieces whose slots fit it; a scan and a gather put the
 * entries in the aligner's order at packed offsets. */
int  bmv_leftalign(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                   const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                   const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint64_t *total_cigar);
/* Results of the last bmv_leftalign: n entries each, out_cigar_offset n + 1, out_cigar total_cigar; any pointer may be NULL. */
int  bmv_leftaligned(bmv_ctx *ctx, uint32_t *out_begin, uint64_t *out_cigar_offset, uint32_t *out_cigar, uint8_t *out_changed,
                     uint32_t *out_dropped);
/* Of the last bmv_leftalign: the kernels' time in ms (walk, scan and gather, all pieces), the columns compared -- every t
 * tested in (2), the one that failed included --, the alignments changed, the merges (3) and the dropped bases.  Any pointer
 * may be NULL. */
int  bmv_last_leftalign_stats(bmv_ctx *ctx, float *ms_kernels, uint64_t *n_compared, uint32_t *n_changed, uint64_t *n_merges,
                              uint64_t *n_dropped);

/* Split alignments: of a read's candidate alignments, the ones that together describe a read spanning a breakpoint (a
 * translocation, a large deletion, a chimeric ligation) -- one primary and up to max_segments - 1 supplementary segments,
 * each candidate cut down to the stretch bmv_clip would keep, no two chosen ones claiming the same part of the read.  A call of
 * its own, of the bmv_annotate / bmv_clip / bmv_pair family: bmv_clip's inputs (the views, begin, M/I/D entries from any align
 * call, match, penalty), groups as bmv_align_best takes them (a group is one read's candidates), contig[a] as in bmv_pair (NULL:
 * one contig), min_score >= 1, max_overlap_permille in 0 .. 1000, 1 <= max_segments <= BMV_SPLIT_MAX_SEGMENTS.  The contract is
 * exact and stated on the outputs only; group size, lane chunking and device count do not show in them.
 * Per alignment a, with m = query_len[a]:
 *   S(a), cl, cr, pos, ref_len   exactly bmv_clip's score, clip_left, clip_right, pos and ref_len for the same inputs (the same
 *                       tie rules: smallest r, then largest l; an empty CIGAR gives zeros, an alignment without an = column
 *                       zeros and cr = m)
 *   q_lo, q_hi          the kept query interval in READ orientation: q_lo = text_rc ? cr : cl, q_hi = m - (text_rc ? cl : cr);
 *                       qlen = q_hi - q_lo
 *   g_lo, g_hi          the kept reference interval in forward genome coordinates, signed 64-bit: g_lo = text_start + pos,
 *                       g_hi = g_lo + ref_len
 *   eligible(a)         S(a) >= min_score
 *   ovl_q(a, b)         max(0, min(q_hi) - max(q_lo)); ovl_g the same on the g intervals
 *   dup(a, b)           same contig, same text_rc, ovl_g > 0 and ovl_q > 0: one alignment found through two windows or buckets
 *   conflict(a, b)      dup(a, b), or ovl_q(a, b) * 1000 > max_overlap_permille * min(qlen(a), qlen(b)), in 64 bits
 * Per group the chosen list C starts empty; while |C| < max_segments: among the eligible a not in C with no conflict(a, c) for
 * any c in C, the one with the greatest S -- the lowest batch index among equals -- is appended; the list ends when there is
 * none.  C[0] is the primary, the rest are supplementary, in that order.  For each chosen c the competitor score s2(c) is the
 * greatest S(a) over the group's a that are not in C, have S(a) > 0, are no dup of c and cover at least half of it
 * (2 * ovl_q(a, c) >= qlen(c)); BMV_SPLIT_NONE when there is none.
 * What is a choice, not a measurement: the pairwise overlap rule, dup, the competitor rule, and ONE range per candidate -- an
 * inversion in the middle of a read keeps one range that spans it and loses the inverted part.
 * Checks before anything is launched: everything bmv_clip refuses, group_offset as in bmv_align_best, the parameter ranges
 * above, text_start below 2^62: BMV_ERR_ARG, the message names the alignment or group, nothing ran and the context stays usable.
 * The call leaves untouched what every other result or stats call returns -- those of bmv_frag_spans, bmv_pair, bmv_rescue,
 * bmv_annotate, bmv_clip, bmv_realign and bmv_leftalign too -- and a pending bmv_paired_begin stays pending; n = 0 and
 * n_groups = 0 succeed with empty results.
 * How (bmv_split.hip.h): the range kernel is bmv_clip's range walk -- a wave per alignment, 64 columns of an M entry a step --
 * carrying the text and query cursors of the running minimum and of the best range along, so that ONE walk gives what bmv_clip
 * takes its range and its count pass for; the pick kernel runs a wave per group, the candidates in the lanes 64 at a time, a
 * round per segment: every candidate is tested again against the chosen intervals (kept one per lane and broadcast), the
 * round's winner is a maximum across the wave, a last sweep gives s2.  Nothing goes back to the host in between. */
#define BMV_SPLIT_MAX_SEGMENTS 16u
#define BMV_SPLIT_NONE INT64_MIN
int  bmv_split(bmv_ctx *ctx, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
               const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
               const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
               uint32_t n_groups, uint32_t match, uint32_t penalty, uint32_t min_score, uint32_t max_overlap_permille,
               uint32_t max_segments);
/* The pick alone, over numbers, as bmv_pair is: score, q_lo, q_hi, g_lo, g_hi as bmv_segments returns them.  In addition to the
 * group and parameter checks: q_lo <= q_hi and g_lo <= g_hi per alignment (BMV_ERR_ARG, the message names the alignment).  It
 * fills the same result row: bmv_segments returns the five arrays as given. */
int  bmv_split_pick(bmv_ctx *ctx, const int64_t *score, const uint32_t *q_lo, const uint32_t *q_hi, const int64_t *g_lo,
                    const int64_t *g_hi, const uint8_t *text_rc, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
                    uint32_t n_groups, uint32_t min_score, uint32_t max_overlap_permille, uint32_t max_segments);
/* Of the last bmv_split or bmv_split_pick: out_score, out_q_lo, out_q_hi, out_g_lo, out_g_hi n entries each; out_n_seg n_groups
 * entries, |C| per group; out_seg and out_s2 n_groups * max_segments entries: the batch indices of group g's chosen alignments
 * in chosen order from g * max_segments on, and their competitor scores; unused slots hold BMV_BEYOND and BMV_SPLIT_NONE.  Any
 * pointer may be NULL. */
int  bmv_segments(bmv_ctx *ctx, int64_t *out_score, uint32_t *out_q_lo, uint32_t *out_q_hi, int64_t *out_g_lo, int64_t *out_g_hi,
                  uint32_t *out_n_seg, uint32_t *out_seg, int64_t *out_s2);
/* Of the last bmv_split or bmv_split_pick: the range kernel's and the pick kernel's time in ms (ms_range 0 after
 * bmv_split_pick), the alignment columns the range kernel walked and the segments chosen in all.  Any pointer may be NULL. */
int  bmv_last_split_stats(bmv_ctx *ctx, float *ms_range, float *ms_pick, uint64_t *n_columns, uint64_t *n_segments);

#ifdef __cplusplus
}
#endif
#endif
