// bucket_locator.h -- exact position inside the candidate buckets + SAM output.
//
// Restates bucket_locator (bucket_map/locator/bucket_locator.h) without SeqAn3.  Host side:
//   query_sequences_storage / _prepare_read_query   :19-103, :292-347
//   _locate: bucket loop and its ordering contract   :613-705
//   _filter_best_locations                           :350-405
//   locate (SAM)                                     :455-611  (both branches: with a verifier plugged
//                                                               in, the BM_ALIGN one)
// The candidate scan itself -- _create_kmer_index (:162-177) + _find_offset (:209-290) for every
// candidate (window, bucket, strand) -- sits behind bm::offset_scanner: the MI355X scan (include/bml.h)
// in the product, the C oracle in the test build.  Order-sensitive details are kept on purpose
// (SURVEY App. A.7): revcomp candidates of a bucket are visited in reverse list order, `offset > 0`
// drops an exact hit at bucket offset 0, results are appended per read in bucket order.
#pragma once

#include "affine_realign.h"
#include "bam.h"
#include "bam_sort.h"
#include "best_mapq.h"
#include "bgzf.h"
#include "bm_genome.h"
#include "frag_range.h"
#include "left_align.h"
#include "overlap_clip.h"
#include "mapper.h"
#include "pair_mapq.h"
#include "pair_rescue.h"
#include "sam_tags.h"
#include "split_pick.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <charconv>
#include <chrono>
#include <iostream>
#include <memory>
#include <string_view>
#include <thread>
#include <tuple>

namespace bm {

// Where _prepare_read_query's sampling and _create_kmer_index + _find_offset run.  One scan call handles
// every candidate of a _locate pass; sampling is called per block of reads.
class offset_scanner {
public:
    virtual ~offset_scanner() = default;
    // _prepare_read_query (:292-347) for windows given as views into bases / quals: p (hash, position) pairs
    // per window, has[w] = 0 for a window shorter than k
    virtual void sample_windows(const uint8_t *bases, const uint8_t *quals, uint64_t n_bytes, const uint64_t *win_start,
                                const uint32_t *win_len, uint32_t n_windows, uint32_t min_base_quality,
                                uint32_t *out_hash, uint16_t *out_pos, uint8_t *out_has) = 0;
    // the same for windows whose bases and qualities lie apart in one buffer (the mapped FASTQ file): window w =
    // text[seq_start[w], +win_len[w]) with qualities text[qual_start[w], +win_len[w]).  Default: gather, then sample_windows.
    virtual void sample_text_windows(const uint8_t *text, uint64_t n_bytes, const uint64_t *seq_start, const uint64_t *qual_start,
                                     const uint32_t *win_len, uint32_t n_windows, uint32_t min_base_quality, uint32_t *out_hash,
                                     uint16_t *out_pos, uint8_t *out_has) {
        (void)n_bytes;
        std::vector<uint64_t> start(n_windows);
        uint64_t at = 0;
        for (uint32_t w = 0; w < n_windows; w++) {
            start[w] = at;
            at += win_len[w];
        }
        std::vector<uint8_t> bases(at + 1), quals(at + 1);
        for (uint32_t w = 0; w < n_windows; w++) {
            std::memcpy(bases.data() + start[w], text + seq_start[w], win_len[w]);
            std::memcpy(quals.data() + start[w], text + qual_start[w], win_len[w]);
        }
        sample_windows(bases.data(), quals.data(), at, start.data(), win_len, n_windows, min_base_quality, out_hash, out_pos, out_has);
    }
    // genome as one byte string; bucket b = [bucket_start[b], +bucket_len[b])
    virtual void load_genome(const uint8_t *bases, uint64_t n_bases, const uint64_t *bucket_start,
                             const uint32_t *bucket_len, uint32_t n_buckets) = 0;
    // ... or from records that are buffers of their own (concatenated in order; bucket_start counts in that concatenation).
    // Default: flatten, then load_genome.
    virtual void load_genome_records(const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records,
                                     const uint64_t *bucket_start, const uint32_t *bucket_len, uint32_t n_buckets) {
        uint64_t total = 0;
        for (uint32_t r = 0; r < n_records; r++) total += rec_len[r];
        std::unique_ptr<uint8_t[]> flat(new uint8_t[total ? total : 1]);
        uint64_t at = 0;
        for (uint32_t r = 0; r < n_records; r++) {
            std::memcpy(flat.get() + at, rec[r], rec_len[r]);
            at += rec_len[r];
        }
        load_genome(flat.get(), total, bucket_start, bucket_len, n_buckets);
    }
    // windows: sample_hash/sample_pos [n_windows x p], seg_len[n_windows]; candidates grouped by bucket.
    // out_offset = what _find_offset returns (first of the pair, or -1), out_votes = second.
    virtual void scan(const uint32_t *sample_hash, const uint16_t *sample_pos, const uint32_t *seg_len,
                      uint32_t n_windows, const uint32_t *pair_bucket, const uint32_t *pair_window,
                      const uint8_t *pair_rc, uint32_t n_pairs, int32_t *out_offset, uint32_t *out_votes) = 0;
};

// Where the BM_ALIGN branch's align_pairwise (:520-528,569) runs: the MI355X verifier (include/bmv.h) in the
// product, the C oracle in the test build.  One call handles a batch of (text window, query) pairs given as
// views into the genome string and into a buffer of reads.
class alignment_verifier {
public:
    virtual ~alignment_verifier() = default;
    virtual void load_genome(const uint8_t *bases, uint64_t n_bases) = 0;
    virtual void load_genome_records(const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records) {
        uint64_t total = 0;
        for (uint32_t r = 0; r < n_records; r++) total += rec_len[r];
        std::unique_ptr<uint8_t[]> flat(new uint8_t[total ? total : 1]);
        uint64_t at = 0;
        for (uint32_t r = 0; r < n_records; r++) {
            std::memcpy(flat.get() + at, rec[r], rec_len[r]);
            at += rec_len[r];
        }
        load_genome(flat.get(), total);
    }
    // score = alignment.score(), begin = sequence1_begin_position(), CIGAR entries packed len << 4 | op
    // (0 M, 1 I, 2 D); alignment a owns cigar[cigar_offset[a] .. cigar_offset[a + 1])
    virtual void align(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                       const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                       std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                       std::vector<uint32_t> &cigar) = 0;
    // The same under an edit bound per alignment (bmv_align_bounded's contract, include/bmv.h): alignment a is kept iff
    // -score <= max_edits[a]; a rejected one comes back with score kRejected, begin 0 and no CIGAR entries.  This default
    // aligns everything and marks the rejections afterwards; the GPU verifier screens first.
    static constexpr int32_t kRejected = INT32_MIN;
    virtual void align_bounded(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                               const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                               const uint32_t *max_edits, uint32_t n, std::vector<int32_t> &score, std::vector<uint32_t> &begin,
                               std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar) {
        align(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, score, begin, cigar_offset, cigar);
        uint64_t at = 0;
        for (uint32_t a = 0; a < n; a++) {
            const uint64_t from = cigar_offset[a], to = cigar_offset[a + 1];
            cigar_offset[a] = at;
            if (-static_cast<int64_t>(score[a]) > static_cast<int64_t>(max_edits[a])) {
                score[a] = kRejected;
                begin[a] = 0;
                continue;
            }
            for (uint64_t x = from; x < to; x++) cigar[at++] = cigar[x];
        }
        cigar_offset[n] = at;
        cigar.resize(at);
    }
    // What a SAM record needs beyond that (bmv_annotate's contract, include/bmv.h): forward-strand pos, =/X/I/D entries, NM
    // and the reference bases under X and D columns, for alignments given with their begin and M/I/D CIGAR.  The GPU
    // verifier's pass; for a verifier without one (can_annotate() false) the locator annotates on the host.
    virtual bool can_annotate() const { return false; }
    virtual void annotate(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                          const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                          const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, annotation &out) {
        (void)reads; (void)n_read_bytes; (void)text_start; (void)text_len; (void)text_rc; (void)query_start; (void)query_len;
        (void)begin; (void)cigar_offset; (void)cigar; (void)n; (void)out;
        throw std::runtime_error("--annotate: this build's alignment verifier has no annotation pass");
    }
    // The same with low-identity ends soft-clipped (bmv_clip's contract, include/bmv.h): the best-scoring contiguous stretch of
    // columns under +match per = column and -penalty per X, I or D column is kept, the rest of the query becomes S entries.
    // The GPU verifier's pass; a verifier without one says so.
    virtual void clip(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                      const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                      const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t penalty,
                      clipping &out) {
        (void)reads; (void)n_read_bytes; (void)text_start; (void)text_len; (void)text_rc; (void)query_start; (void)query_len;
        (void)begin; (void)cigar_offset; (void)cigar; (void)n; (void)match; (void)penalty; (void)out;
        throw std::runtime_error("--clip: this build's alignment verifier has no clipping pass");
    }
    // The same for pairs (bmv_overlap's contract, include/bmv.h): clip's record -- all columns kept when match == penalty == 0 --,
    // and where the two mates of a pair (mate[a]: the index of a's mate, overlap::kNoMate for none; contig: per alignment, or null
    // for one contig) overlap on the reference without containment, both soft-clipped at one cut so that no base lies under both.
    // cut[a]: the query bases the cut clipped; pairs_cut, bases_cut: the pairs cut and the sum of cut.  This default restates the
    // rule on the host (overlap_clip.h), whatever the scores, and needs `genome` as realign's does; the GPU verifier clips on the
    // device (can_clip_overlap() true) and ignores it.
    virtual bool can_clip_overlap() const { return false; }
    virtual void clip_overlap(const uint8_t *genome, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                              const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                              const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *mate,
                              const uint32_t *contig, uint32_t n, uint32_t match, uint32_t penalty, clipping &out,
                              std::vector<uint32_t> &cut, uint64_t &pairs_cut, uint64_t &bases_cut) {
        (void)n_read_bytes;
        clip_overlap_on_host(genome, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, mate, contig, n,
                             match, penalty, out, cut, pairs_cut, bases_cut);
    }
    // Split alignments (bmv_split's contract, include/bmv.h): per alignment the stretch clip would keep as a query interval in read
    // orientation and a reference interval in genome coordinates, per group -- a read's candidates -- the non-conflicting
    // stretches in chosen order with their competitor scores.  contig: per alignment, or null for one contig.  The rule rests
    // on the clipping pass, so it is the GPU verifier's; a verifier without one says so.
    virtual void split(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                       const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                       const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
                       uint32_t n_groups, const split_params &params, split_result &out) {
        (void)reads; (void)n_read_bytes; (void)text_start; (void)text_len; (void)text_rc; (void)query_start; (void)query_len;
        (void)begin; (void)cigar_offset; (void)cigar; (void)contig; (void)n; (void)group_offset; (void)n_groups; (void)params; (void)out;
        throw std::runtime_error("--split: this build's alignment verifier has no clipping pass to split by");
    }
    // The affine-gap realignment of alignments given with their begin and M/I/D CIGAR (bmv_realign's contract, include/bmv.h):
    // per alignment the score, begin and entries of the best path inside the band that follows the given one, or -- passed
    // through -- the given path with its affine score.  This default computes the contract on the host (affine_realign.h) and
    // needs `genome`, the records back to back as the verifier's own copy lies; the GPU verifier realigns on the device
    // (can_realign() true) and ignores it.
    virtual bool can_realign() const { return false; }
    virtual void realign(const uint8_t *genome, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                         const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                         const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n,
                         const affine_scores &scores, realignment &out) {
        (void)n_read_bytes;
        affine::realign_on_host(genome, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, n, scores,
                                out);
    }
    // Every I and D entry of alignments given with their begin and M/I/D CIGAR moved to its leftmost equivalent place on the
    // forward strand (bmv_leftalign's contract, include/bmv.h).  This default restates the rule on the host (left_align.h) and
    // needs `genome` as realign's does; the GPU verifier normalises on the device (can_left_align() true) and ignores it.
    virtual bool can_left_align() const { return false; }
    virtual void left_align(const uint8_t *genome, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                            const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                            const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, left_alignment &out) {
        (void)n_read_bytes;
        leftalign::left_align_on_host(genome, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, n, out);
    }
    // The best alignment of every group (bmv_align_best's contract, include/bmv.h): group g owns the alignments
    // group_offset[g] .. group_offset[g + 1] - 1; with d = -score and end = begin + the M and D lengths, winner[g] is the lowest
    // index with the group's smallest d (kBeyond for an empty group) and alone keeps its score, begin and CIGAR -- every other
    // alignment comes back with score kRejected, begin 0 and no entries; edits / end carry d / end of every alignment with
    // d <= best + margin[g], kBeyond / 0 elsewhere.  hint[g] (may be null) is the index inside the group to try first; the
    // result does not depend on it.  This default aligns everything and selects afterwards; the GPU verifier aligns one
    // alignment per group in full and decides the rest score-only.
    static constexpr uint32_t kBeyond = UINT32_MAX;
    virtual void best(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                      const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                      const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                      std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                      std::vector<uint32_t> &cigar, std::vector<uint32_t> &winner, std::vector<uint32_t> &edits,
                      std::vector<uint32_t> &end) {
        (void)hint;
        align(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, score, begin, cigar_offset, cigar);
        std::vector<uint32_t> d(n), e(n);
        for (uint32_t a = 0; a < n; a++) {
            uint32_t r = 0;
            for (uint64_t x = cigar_offset[a]; x < cigar_offset[a + 1]; x++)
                if ((cigar[x] & 15u) != 1u) r += cigar[x] >> 4;
            d[a] = static_cast<uint32_t>(-static_cast<int64_t>(score[a]));
            e[a] = begin[a] + r;
        }
        winner.assign(n_groups, kBeyond);
        edits.assign(n, kBeyond);
        end.assign(n, 0);
        std::vector<uint8_t> wins(n, 0);
        for (uint32_t g = 0; g < n_groups; g++) {
            const uint32_t a0 = group_offset[g], a1 = group_offset[g + 1];
            if (a0 == a1) continue;
            uint32_t w = a0;
            for (uint32_t a = a0 + 1; a < a1; a++)
                if (d[a] < d[w]) w = a;
            winner[g] = w;
            wins[w] = 1;
            const uint64_t reach = static_cast<uint64_t>(d[w]) + margin[g];
            for (uint32_t a = a0; a < a1; a++) {
                if (d[a] > reach) continue;
                edits[a] = d[a];
                end[a] = e[a];
            }
        }
        uint64_t at = 0;
        for (uint32_t a = 0; a < n; a++) {
            const uint64_t from = cigar_offset[a], to = cigar_offset[a + 1];
            cigar_offset[a] = at;
            if (!wins[a]) {
                score[a] = kRejected;
                begin[a] = 0;
                continue;
            }
            for (uint64_t x = from; x < to; x++) cigar[at++] = cigar[x];
        }
        cigar_offset[n] = at;
        cigar.resize(at);
    }
    // The same for pairs (bmv_align_paired's contract, include/bmv.h): the groups 2p and 2p + 1 are the candidates of the two
    // mates of pair p (n_groups is even); winner, edits and end as best() returns them; pick[g] is the alignment of group g that
    // select_pair (pair_mapq.h) picks over those edits and ends -- the group's own winner where the pair has no proper
    // combination -- and alone keeps its score, begin and CIGAR; proper, s1 and s2 per pair.  contig[a] (may be null: one
    // contig) is the reference sequence alignment a lies on.  This default aligns everything and picks on the host; the GPU
    // verifier aligns in full only the seeds and the picks.
    virtual void paired(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                        const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                        const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                        const uint32_t *contig, uint32_t min_frag, uint32_t max_frag, std::vector<int32_t> &score,
                        std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar,
                        std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end,
                        std::vector<uint32_t> &pick, std::vector<uint8_t> &proper, std::vector<uint64_t> &s1, std::vector<uint64_t> &s2) {
        (void)hint;
        if (n_groups & 1u) throw std::runtime_error("paired: an odd number of groups");
        paired_distances(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, group_offset, n_groups, margin, score,
                         begin, cigar_offset, cigar, winner, edits, end);
        paired_pick(text_start, text_len, text_rc, query_len, n, group_offset, n_groups, contig, min_frag, max_frag, score, begin, cigar_offset,
                    cigar, edits, end, pick, proper, s1, s2);
    }
    // What a learned range was made of: the applied range, whether it was learned (else it is the fallback), the informative
    // pairs and the three quartiles (0 when not learned).
    struct frag_learned {
        uint32_t applied_min = 0, applied_max = 0;
        bool learned = false;
        uint64_t n_informative = 0;
        uint32_t quartiles[3] = {0, 0, 0};
    };
    // paired() under a range learned from the batch itself (bmv_frag_spans' contract, include/bmv.h, and frag_range.h): the
    // spans of the batch's pairs under `cap`, their histogram, bm::frag_range with min_pairs and the fallback range, then the
    // pick under the applied range.  Everything paired() returns, plus what was learned.  This default aligns everything and
    // does the rest on the host; the GPU verifier leaves a histogram per device, adds them and picks on every device under the
    // one range.
    virtual void paired_auto(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                             const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                             const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                             const uint32_t *contig, uint32_t cap, uint32_t min_pairs, uint32_t fallback_min, uint32_t fallback_max,
                             std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                             std::vector<uint32_t> &cigar, std::vector<uint32_t> &winner, std::vector<uint32_t> &edits,
                             std::vector<uint32_t> &end, std::vector<uint32_t> &pick, std::vector<uint8_t> &proper, std::vector<uint64_t> &s1,
                             std::vector<uint64_t> &s2, frag_learned &learned) {
        (void)hint;
        if (n_groups & 1u) throw std::runtime_error("paired: an odd number of groups");
        if (cap < 1u || cap > 65535u) throw std::runtime_error("paired: a fragment cap is 1 .. 65535");
        paired_distances(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, group_offset, n_groups, margin, score,
                         begin, cigar_offset, cigar, winner, edits, end);
        std::vector<uint64_t> hist(static_cast<size_t>(cap) + 1u, 0);
        for (uint32_t p = 0; p < n_groups / 2u; p++)
            hist[frag_span(text_start, text_len, text_rc, query_len, edits.data(), end.data(), contig, group_offset[2 * p],
                           group_offset[2 * p + 1], group_offset[2 * p + 2], cap)]++;
        learned = learn(hist, min_pairs, fallback_min, fallback_max);
        paired_pick(text_start, text_len, text_rc, query_len, n, group_offset, n_groups, contig, learned.applied_min, learned.applied_max, score,
                    begin, cigar_offset, cigar, edits, end, pick, proper, s1, s2);
    }

protected:
    static frag_learned learn(const std::vector<uint64_t> &hist, uint32_t min_pairs, uint32_t fallback_min, uint32_t fallback_max) {
        const frag_range_result r = frag_range(hist.data(), hist.size(), min_pairs, fallback_min, fallback_max);
        frag_learned out;
        out.applied_min = r.min_frag;
        out.applied_max = r.max_frag;
        out.learned = r.learned;
        out.n_informative = r.n_informative;
        out.quartiles[0] = r.q1;
        out.quartiles[1] = r.q2;
        out.quartiles[2] = r.q3;
        return out;
    }

private:
    // the default paired()'s first step: everything aligned, (edits, end) restricted to best + margin per group
    void paired_distances(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                          const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                          const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, std::vector<int32_t> &score,
                          std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar,
                          std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end) {
        align(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, score, begin, cigar_offset, cigar);
        winner.assign(n_groups, kBeyond);
        edits.assign(n, kBeyond);
        end.assign(n, 0);
        for (uint32_t g = 0; g < n_groups; g++) {
            const uint32_t a0 = group_offset[g], a1 = group_offset[g + 1];
            uint64_t best_d = UINT64_MAX;
            for (uint32_t a = a0; a < a1; a++) best_d = std::min<uint64_t>(best_d, static_cast<uint64_t>(-static_cast<int64_t>(score[a])));
            for (uint32_t a = a0; a < a1; a++) {
                const uint64_t d = static_cast<uint64_t>(-static_cast<int64_t>(score[a]));
                if (d == best_d && winner[g] == kBeyond) winner[g] = a;
                if (d > best_d + margin[g]) continue;
                uint32_t r = 0;
                for (uint64_t x = cigar_offset[a]; x < cigar_offset[a + 1]; x++)
                    if ((cigar[x] & 15u) != 1u) r += cigar[x] >> 4;
                edits[a] = static_cast<uint32_t>(d);
                end[a] = begin[a] + r;
            }
        }
    }
    // ... and its second: the pick under a range, and only the picks keep their results
    void paired_pick(const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len, uint32_t n,
                     const uint32_t *group_offset, uint32_t n_groups, const uint32_t *contig, uint32_t min_frag, uint32_t max_frag,
                     std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                     std::vector<uint32_t> &cigar, const std::vector<uint32_t> &edits, const std::vector<uint32_t> &end,
                     std::vector<uint32_t> &pick, std::vector<uint8_t> &proper, std::vector<uint64_t> &s1, std::vector<uint64_t> &s2) {
        pick.assign(n_groups, kBeyond);
        proper.assign(n_groups / 2u, 0);
        s1.assign(n_groups / 2u, kPairNone);
        s2.assign(n_groups / 2u, kPairNone);
        std::vector<uint8_t> keep(n, 0);
        for (uint32_t p = 0; p < n_groups / 2u; p++) {
            const pair_pick pp = select_pair(text_start, text_len, text_rc, query_len, edits.data(), end.data(), contig, group_offset[2 * p],
                                             group_offset[2 * p + 1], group_offset[2 * p + 2], min_frag, max_frag);
            for (uint32_t k = 0; k < 2u; k++) {
                pick[2 * p + k] = pp.pick[k];
                if (pp.pick[k] != kBeyond) keep[pp.pick[k]] = 1;
            }
            proper[p] = pp.proper ? 1 : 0;
            s1[p] = pp.s1;
            s2[p] = pp.s2;
        }
        uint64_t at = 0;
        for (uint32_t a = 0; a < n; a++) {
            const uint64_t from = cigar_offset[a], to = cigar_offset[a + 1];
            cigar_offset[a] = at;
            if (!keep[a]) {
                score[a] = kRejected;
                begin[a] = 0;
                continue;
            }
            for (uint64_t x = from; x < to; x++) cigar[at++] = cigar[x];
        }
        cigar_offset[n] = at;
        cigar.resize(at);
    }

public:
    // Mate rescue (bmv_rescue's contract, include/bmv.h): job j places the mate reads[query_start[j], +query_len[j]) beside its
    // anchor -- a known alignment of its partner, given as select_pair takes one -- on the contig [contig_start[j],
    // contig_end[j]), within max_edits[j] edits.  out: the view of pair_rescue.h's rescue_window per job, edits / end the
    // query's distance to it and its end column when within min(max_edits, query_len) (kBeyond / 0 elsewhere, and for an
    // empty view or query), proper as select_pair's between the anchor and the rescued mate.  This default plans on the host
    // and aligns every view in full; the GPU verifier plans and decides score-only on the device.
    struct rescued {
        std::vector<uint64_t> text_start;
        std::vector<uint32_t> text_len, edits, end;
        std::vector<uint8_t> text_rc, proper;
    };
    virtual void rescue(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *anchor_text_start, const uint32_t *anchor_text_len,
                        const uint8_t *anchor_text_rc, const uint32_t *anchor_query_len, const uint32_t *anchor_end,
                        const uint64_t *contig_start, const uint64_t *contig_end, const uint64_t *query_start, const uint32_t *query_len,
                        const uint32_t *max_edits, uint32_t n, uint32_t min_frag, uint32_t max_frag, rescued &out) {
        out.text_start.assign(n, 0);
        out.text_len.assign(n, 0);
        out.text_rc.assign(n, 0);
        out.edits.assign(n, kBeyond);
        out.end.assign(n, 0);
        out.proper.assign(n, 0);
        std::vector<uint32_t> which, tl, ql;
        std::vector<uint64_t> ts, qs;
        std::vector<uint8_t> trc;
        for (uint32_t j = 0; j < n; j++) {
            const rescue_view v = rescue_window(anchor_text_start[j], anchor_text_len[j], anchor_text_rc[j] != 0, anchor_query_len[j],
                                                anchor_end[j], contig_start[j], contig_end[j], query_len[j], max_edits[j], min_frag, max_frag);
            out.text_start[j] = v.text_start;
            out.text_len[j] = v.text_len;
            out.text_rc[j] = v.text_rc;
            if (v.text_len == 0 || query_len[j] == 0) continue;
            which.push_back(j);
            ts.push_back(v.text_start); tl.push_back(v.text_len); trc.push_back(v.text_rc);
            qs.push_back(query_start[j]); ql.push_back(query_len[j]);
        }
        std::vector<int32_t> score;
        std::vector<uint32_t> begin, cigar;
        std::vector<uint64_t> cigar_offset;
        if (!which.empty())
            align(reads, n_read_bytes, ts.data(), tl.data(), trc.data(), qs.data(), ql.data(), static_cast<uint32_t>(which.size()), score, begin,
                  cigar_offset, cigar);
        for (size_t s = 0; s < which.size(); s++) {
            const uint32_t j = which[s];
            const uint64_t d = static_cast<uint64_t>(-static_cast<int64_t>(score[s]));
            if (d > std::min(max_edits[j], query_len[j])) continue;
            uint32_t r = 0;
            for (uint64_t x = cigar_offset[s]; x < cigar_offset[s + 1]; x++)
                if ((cigar[x] & 15u) != 1u) r += cigar[x] >> 4;
            out.edits[j] = static_cast<uint32_t>(d);
            out.end[j] = begin[s] + r;
            out.proper[j] = rescue_proper(anchor_text_start[j], anchor_text_len[j], anchor_text_rc[j] != 0, anchor_query_len[j], anchor_end[j],
                                          rescue_view{out.text_start[j], out.text_len[j], out.text_rc[j]}, query_len[j], out.end[j], min_frag,
                                          max_frag) ? 1 : 0;
        }
    }
};

// SAM text as seqan3::sam_file_output lays it out: records are appended to one buffer with
// std::to_chars and go to the file a few megabytes at a time (a million `ostream <<` chains were the slowest stage
// of the tool after the device work had shrunk to milliseconds).
//
// With a block_compressor the same records leave as BAM (-o x.bam): flush() encodes the buffer's complete lines
// (host/bam.h), cuts the BAM stream every kBgzfBlockMax bytes -- by size alone, so the file does not depend on where the
// flushes fell -- and hands the whole blocks to the compressor in one call (the device in the product, host/bgzf.h
// elsewhere; the same bytes); the remainder is carried to the next flush, the header is a block of its own and close()
// appends the BGZF end-of-file block.
//
// Sorted (-o x.bam --sort, host/bam_sort.h): the encoded records are not cut into blocks but kept by a bam_sorter, the
// header says SO:coordinate, and close() writes the records in coordinate order, the EOF block and x.bam.bai.
// --vcf: the file, the rule's parameters, the QUAL (phred) below which a call is LowQual and the sample's name
struct vcf_options {
    std::filesystem::path file;
    genotype_params params{};
    uint32_t min_qual = 20;
    std::string sample = "sample";
    bool indels = false;            // --vcf-indels: the indel calls of include/bmn.h, merged into the file by (reference, POS)
    indel_params indel{};
    std::filesystem::path gvcf;     // --gvcf: the same calls and the reference blocks of include/bmr.h between them; with or without `file`
    std::vector<uint32_t> gvcf_bands;
    bool bias = false;              // --vcf-bias: FS, MQ, ADF and ADR on the SNV lines (include/bmb.h); tables are bmb_tables's
    std::shared_ptr<const bias_tables> bias_tables_of;
    uint32_t max_fs = 60, min_mq = 0;
    bool phase = false;             // --vcf-phase: read-backed phase of the het SNV lines (include/bmk.h); min_mapq and min_bq are `params`'s
    phase_params phase_params_of{};
    bool on() const { return !file.empty() || !gvcf.empty(); }
};

class sam_text {
    std::ofstream out_;
    std::string buf_, writing_;     // the buffer being filled / the one a writer thread is putting into the file
    std::thread writer_;
    bool write_failed_ = false;
    block_compressor *bam_ = nullptr;   // non-null: BAM
    bam_ref_index ref_index_;
    std::string stream_;                // BAM: encoded records not yet in a block
    std::vector<uint8_t> blocks_;
    bool closed_ = false;
    std::unique_ptr<bam_sorter> sorter_;   // non-null: sorted BAM
    uint64_t header_bytes_ = 0;            // sorted BAM: the header's blocks in the file
    size_t n_ref_ = 0;
    bool markdup_ = false;                 // sorted BAM: duplicates flagged
    std::filesystem::path depth_file_, coverage_file_;   // sorted BAM: --depth / --coverage, either may be empty
    std::vector<std::string> ref_ids_;     // ... the references, for the two files
    std::vector<uint32_t> ref_len_;
    std::filesystem::path pileup_file_;    // sorted BAM: --pileup, may be empty
    pileup_thresholds pileup_thresholds_;
    const std::vector<std::string> *pileup_seqs_ = nullptr;   // ... the bases of the header's references, each of its length
    vcf_options vcf_;                      // sorted BAM: --vcf, its file may be empty; it counts the pileup whether that has a file or not
    bool pileup_on() const { return !pileup_file_.empty() || vcf_.on(); }
    std::filesystem::path stats_file_;     // sorted BAM: --stats, may be empty
    stats_params stats_params_;

    // A file of --depth / --coverage / --pileup: written beside its place and moved there when it is complete, so that a failure
    // leaves nothing half-written (and nothing at all under the final name).
    template <typename Fill>
    static void write_whole(const std::filesystem::path &file, Fill &&fill) {
        const std::filesystem::path tmp = file.string() + ".tmp";
        try {
            std::ofstream f(tmp, std::ios::binary);
            if (!f) throw std::runtime_error("cannot write " + file.string());
            fill(f);
            f.close();
            if (!f) throw std::runtime_error("writing " + file.string() + " failed");
            std::filesystem::rename(tmp, file);
        } catch (...) {
            std::error_code ec;
            std::filesystem::remove(tmp, ec);
            throw;
        }
    }
    void write_depth_files() {
        const depth_result &res = sorter_->depth();
        if (!depth_file_.empty()) write_whole(depth_file_, [&](std::ostream &f) { write_depth_file(f, res, ref_ids_); });
        if (!coverage_file_.empty()) write_whole(coverage_file_, [&](std::ostream &f) { write_coverage_file(f, res, ref_ids_, ref_len_); });
        uint64_t cov = 0, bases = 0, reads = 0, n_long = 0;
        for (size_t r = 0; r < ref_len_.size(); r++) {
            const uint64_t *st = res.stats.data() + r * kDepthStats;
            cov += st[1], bases += ref_len_[r], reads += st[0], n_long += st[6];
        }
        std::cerr << "[INFO]\t\tCoverage: " << cov << " of " << bases << " bases covered by " << reads << " records (" << n_long
                  << " long-CIGAR records left out)\n";
    }
    void write_stats() {
        const stats_result &res = sorter_->stats();
        write_whole(stats_file_, [&](std::ostream &f) { write_stats_file(f, res); });
        std::cerr << "[INFO]\t\t" << stats_summary_line(res) << "\n";
    }
    void write_vcf() {
        const genotype_result &res = sorter_->genotype();
        std::vector<uint32_t> lens;
        for (size_t r = 0; r < ref_ids_.size(); r++) lens.push_back((*pileup_seqs_)[r].size());   // set_pileup has checked them
        vcf_bias noted;                                  // --vcf-bias: one annotation per call
        if (vcf_.bias) noted.notes = sorter_->bias_notes(), noted.max_fs = vcf_.max_fs, noted.min_mq = vcf_.min_mq;
        const vcf_bias *bias = vcf_.bias ? &noted : nullptr;
        vcf_phase linked;                                // --vcf-phase: eight words per het SNV call
        if (vcf_.phase) linked.sites = sorter_->phase().sites, linked.index(res.n_calls());
        const vcf_phase *phase = vcf_.phase ? &linked : nullptr;
        // with --gvcf alone there is no file of --vcf: the calls go into the gVCF only
        if (!vcf_.file.empty() && !vcf_.indels) write_whole(vcf_.file, [&](std::ostream &f) { write_vcf_file(f, res, ref_ids_, lens, vcf_.sample, vcf_.min_qual, nullptr, nullptr, nullptr, bias, phase); });
        else if (!vcf_.file.empty()) {
            // the indel lines go between the SNV lines by (reference, POS); at an equal POS the SNV comes first
            const indel_result &ind = sorter_->indel();
            size_t next = 0;
            const vcf_between between = [&](std::string &buf, uint32_t ref, uint64_t pos) {
                for (; next < ind.n_calls(); next++) {
                    const uint32_t *c = ind.calls.data() + kIndelCallWords * next;
                    if (c[0] > ref || (c[0] == ref && static_cast<uint64_t>(c[1]) + 1 >= pos)) break;
                    if (c[5] & kIndelVariant) append_indel_vcf_line(buf, c, ref_ids_.at(c[0]), (*pileup_seqs_)[c[0]], vcf_.min_qual);
                }
            };
            write_whole(vcf_.file, [&](std::ostream &f) {
                next = 0;
                write_vcf_file(f, res, ref_ids_, lens, vcf_.sample, vcf_.min_qual, indel_vcf_header(), &between, nullptr, bias, phase);
            });
        }
        const genotype_summary s = summarize_genotypes(res, vcf_.min_qual);
        std::cerr << "[INFO]\t\tGenotypes: " << s.variants << " variants (" << s.het << " het, " << s.hom << " hom, " << s.low_qual
                  << " below QUAL) at " << res.n_snv_sites << " SNV sites\n";
        if (vcf_.indels) std::cerr << "[INFO]\t\t" << indel_summary_line(summarize_indels(sorter_->indel(), vcf_.min_qual)) << "\n";
        if (!vcf_.gvcf.empty()) write_gvcf(res, lens, bias, phase);
        if (bias) std::cerr << "[INFO]\t\t" << bias_summary_line(summarize_bias(noted)) << "\n";
        if (phase) std::cerr << "[INFO]\t\t" << phase_summary_line(summarize_phase(sorter_->phase(), res.calls.data())) << "\n";
    }
    // --gvcf: the lines of --vcf, and between them by (reference, POS) one line per reference block.  No two lines share a POS:
    // the position of every variant line is excluded from the blocks.
    void write_gvcf(const genotype_result &res, const std::vector<uint32_t> &lens, const vcf_bias *bias, const vcf_phase *phase) {
        const refblock_result &blk = sorter_->refblocks();
        const indel_result &ind = sorter_->indel();
        size_t next = 0, next_block = 0;
        const vcf_between between = [&](std::string &buf, uint32_t ref, uint64_t pos) {
            for (;;) {
                while (vcf_.indels && next < ind.n_calls() && !(ind.calls[kIndelCallWords * next + 5] & kIndelVariant)) next++;
                const uint32_t *c = vcf_.indels && next < ind.n_calls() ? ind.calls.data() + kIndelCallWords * next : nullptr;
                const uint32_t *b = next_block < blk.n_blocks() ? blk.blocks.data() + kRefBlockWords * next_block : nullptr;
                if (c && (c[0] > ref || (c[0] == ref && static_cast<uint64_t>(c[1]) + 1 >= pos))) c = nullptr;
                if (b && (b[0] > ref || (b[0] == ref && static_cast<uint64_t>(b[1]) + 1 >= pos))) b = nullptr;
                if (!c && !b) break;
                if (c && (!b || c[0] < b[0] || (c[0] == b[0] && c[1] <= b[1])))
                    append_indel_vcf_line(buf, c, ref_ids_.at(c[0]), (*pileup_seqs_)[c[0]], vcf_.min_qual), next++;
                else
                    append_block_line(buf, b, ref_ids_.at(b[0]), reinterpret_cast<const uint8_t *>((*pileup_seqs_)[b[0]].data())), next_block++;
            }
        };
        const char *const more[3] = {gvcf_alt_header(), gvcf_info_header(), gvcf_format_header()};
        write_whole(vcf_.gvcf, [&](std::ostream &f) {
            next = next_block = 0;
            write_vcf_file(f, res, ref_ids_, lens, vcf_.sample, vcf_.min_qual, vcf_.indels ? indel_vcf_header() : nullptr, &between, more, bias, phase);
        });
        std::cerr << "[INFO]\t\t" << refblock_summary_line(blk, lens) << "\n";
    }
    void write_pileup() {
        const pileup_result &res = sorter_->pileup();
        write_whole(pileup_file_, [&](std::ostream &f) { write_pileup_file(f, res, ref_ids_); });
        uint64_t sites = 0, bases = 0, reads = 0, left_out = 0, low_mapq = 0;
        for (size_t r = 0; r < ref_ids_.size(); r++) {
            const uint64_t *st = res.stats.data() + r * kPileupStats;
            reads += st[0], low_mapq += st[1], left_out += st[2], bases += st[3], sites += st[5];
        }
        std::cerr << "[INFO]\t\tPileup: " << sites << " sites on " << bases << " bases from " << reads << " records (" << left_out
                  << " left out, " << low_mapq << " below MAPQ)\n";
    }
    // --pileup: the references' bases for the sorter, one string of the header's length per reference
    void set_pileup(const std::vector<std::string> &ref_ids, const std::vector<size_t> &ref_lengths) {
        if (!pileup_seqs_ || pileup_seqs_->size() != ref_ids.size())
            throw std::runtime_error("--pileup: " + std::to_string(pileup_seqs_ ? pileup_seqs_->size() : 0) + " sequences for the " +
                                     std::to_string(ref_ids.size()) + " references of the header");
        std::vector<const uint8_t *> bases(ref_ids.size());
        for (size_t r = 0; r < ref_ids.size(); r++) {
            const std::string &seq = (*pileup_seqs_)[r];
            if (seq.size() != ref_lengths[r])
                throw std::runtime_error("--pileup: " + std::to_string(seq.size()) + " bases for " + ref_ids[r] + ", which has " +
                                         std::to_string(ref_lengths[r]));
            bases[r] = reinterpret_cast<const uint8_t *>(seq.data());
        }
        sorter_->set_pileup(ref_lengths, bases, pileup_thresholds_);
        if (vcf_.on()) sorter_->set_genotype(vcf_.params);
        if (vcf_.on() && vcf_.indels) sorter_->set_indel(vcf_.indel);
        if (!vcf_.gvcf.empty()) sorter_->set_refblocks(vcf_.gvcf_bands);
        if (vcf_.on() && vcf_.bias) {
            if (!vcf_.bias_tables_of) throw std::runtime_error("--vcf-bias: no tables");
            sorter_->set_bias(bias_params{vcf_.params.min_mapq, vcf_.params.min_bq}, *vcf_.bias_tables_of);
        }
        if (vcf_.on() && vcf_.phase) {
            phase_params pr = vcf_.phase_params_of;
            pr.min_mapq = vcf_.params.min_mapq, pr.min_bq = vcf_.params.min_bq;
            sorter_->set_phase(pr);
        }
    }

    // BAM: buf_ (whole lines) -> records -> the whole blocks among them (all of them when `all`), left in buf_ for the writer
    void encode_buffer(bool all) {
        // a few threads, each a run of whole lines; their records are appended in order (one thread encodes 640 MB of
        // text in half a second: as long as the device takes for everything else)
        // (BM_BAM_ENCODE_BYTES: the text size from which a flush is shared out, for the tests; default 1 MiB)
        static const size_t share_from = [] {
            const char *e = std::getenv("BM_BAM_ENCODE_BYTES");
            return e ? static_cast<size_t>(std::strtoull(e, nullptr, 10)) : size_t{1} << 20;
        }();
        const unsigned T = buf_.size() < share_from ? 1u : std::min(8u, std::max(2u, std::thread::hardware_concurrency()));
        std::vector<size_t> cut(T + 1, buf_.size());
        cut[0] = 0;
        for (unsigned t = 1; t < T; t++) {
            const size_t nl = buf_.find('\n', std::max(cut[t - 1], buf_.size() / T * t));
            cut[t] = nl == std::string::npos ? buf_.size() : nl + 1;
        }
        std::vector<std::string> part(T);
        std::vector<std::exception_ptr> failed(T);
        auto encode = [&](unsigned t) {
            try {
                for (size_t at = cut[t]; at < cut[t + 1];) {
                    size_t e = buf_.find('\n', at);
                    if (e == std::string::npos) e = buf_.size();
                    sam_line_to_bam(std::string_view(buf_).substr(at, e - at), ref_index_, t ? part[t] : stream_);
                    at = e + 1;
                }
            } catch (...) {
                failed[t] = std::current_exception();
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < T; t++) pool.emplace_back(encode, t);
        encode(0);
        for (auto &th : pool) th.join();
        for (unsigned t = 0; t < T; t++)
            if (failed[t]) std::rethrow_exception(failed[t]);
        for (unsigned t = 1; t < T; t++) stream_.append(part[t]);
        if (sorter_) {                                // sorted: the records wait for close(), nothing goes to the file yet
            sorter_->add(reinterpret_cast<const uint8_t *>(stream_.data()), stream_.size());
            stream_.clear();
            buf_.clear();
            return;
        }
        const size_t take = all ? stream_.size() : stream_.size() / kBgzfBlockMax * kBgzfBlockMax;
        blocks_.clear();
        if (take) bam_->deflate(reinterpret_cast<const uint8_t *>(stream_.data()), take, blocks_);
        stream_.erase(0, take);
        buf_.assign(reinterpret_cast<const char *>(blocks_.data()), blocks_.size());
    }

    void join_writer() {
        if (writer_.joinable()) writer_.join();
        if (write_failed_) throw std::runtime_error("writing the SAM file failed");
    }

    static void number(std::string &buf, uint64_t v) {
        char tmp[24];
        const auto r = std::to_chars(tmp, tmp + sizeof tmp, v);
        buf.append(tmp, static_cast<size_t>(r.ptr - tmp));
    }
    void number(uint64_t v) { number(buf_, v); }

public:
    // sort_run_bytes > 0 (BAM only): coordinate-sorted output in runs of that many bytes of BAM stream; markdup: the
    // duplicates among the records are flagged 0x400 on the way (--markdup, include/bmd.h)
    // depth_file / coverage_file (sorted BAM only, either may be empty): the bedGraph runs of equal depth and the table per
    // reference of the records written (--depth, --coverage, include/bmc.h)
    // pileup_file (sorted BAM only, may be empty): the table of variant sites of the records written (--pileup, include/bmp.h),
    // under these thresholds and against ref_bases, the bases of the header's references (each as long as the header says)
    // vcf (sorted BAM only, its file may be empty): the genotypes at the pileup's SNV sites as a VCF file (--vcf, include/bmg.h);
    // it counts the pileup under pileup_th with or without a pileup_file
    explicit sam_text(std::filesystem::path const &file, block_compressor *bam = nullptr, size_t sort_run_bytes = 0, bool markdup = false,
                      std::filesystem::path const &depth_file = {}, std::filesystem::path const &coverage_file = {},
                      std::filesystem::path const &pileup_file = {}, pileup_thresholds const &pileup_th = {},
                      const std::vector<std::string> *ref_bases = nullptr, vcf_options const &vcf = {})
        : out_(file, std::ios::binary), bam_(bam), pileup_thresholds_(pileup_th), pileup_seqs_(ref_bases), vcf_(vcf) {
        if (!out_) throw std::runtime_error("cannot write " + file.string());
        if (bam_ && sort_run_bytes) sorter_ = std::make_unique<bam_sorter>(bam_, file, sort_run_bytes, markdup);
        markdup_ = sorter_ && markdup;
        depth_file_ = sorter_ ? depth_file : std::filesystem::path();
        coverage_file_ = sorter_ ? coverage_file : std::filesystem::path();
        pileup_file_ = sorter_ ? pileup_file : std::filesystem::path();
        if (!sorter_) vcf_.file.clear(), vcf_.gvcf.clear();
        buf_.reserve(5u << 20);
        writing_.reserve(5u << 20);
    }
    // --stats FILE (sorted BAM only, before header()): the mapping statistics of the records written (include/bmq.h)
    void set_stats(std::filesystem::path const &file, stats_params const &pr) {
        stats_file_ = sorter_ ? file : std::filesystem::path();
        stats_params_ = pr;
    }
    ~sam_text() {
        try {
            if (!closed_) flush();
            join_writer();
        } catch (...) {
        }
    }
    // the filled buffer goes to the file on a thread of its own while the next one is filled (records are formatted at
    // about the speed the file system takes them: one after the other they cost twice)
    void flush() {
        if (bam_) encode_buffer(false);
        join_writer();
        writing_.swap(buf_);
        buf_.clear();
        writer_ = std::thread([this]() {
            out_.write(writing_.data(), static_cast<std::streamsize>(writing_.size()));
            if (!out_) write_failed_ = true;
        });
    }
    // everything written (call before reading the file back or reporting success)
    void close() {
        if (sorter_ && !closed_) {
            encode_buffer(true);
            join_writer();
            sorter_->finish(out_, header_bytes_, n_ref_);
            std::cerr << "[INFO]\t\tSorted " << sorter_->n_records() << " records by coordinate in " << sorter_->n_runs() << " run(s), "
                      << sorter_->n_passes() << " radix pass(es) on the device.\n";
            if (markdup_) {
                const uint64_t *c = sorter_->dup_counts();
                std::cerr << "[INFO]\t\tMarked " << c[2] + c[3] << " of " << sorter_->n_records() << " records as duplicates (" << c[0]
                          << " pair units, " << c[1] << " fragment units)\n";
            }
            if (!depth_file_.empty() || !coverage_file_.empty()) write_depth_files();
            if (!pileup_file_.empty()) write_pileup();
            if (vcf_.on()) write_vcf();
            if (!stats_file_.empty()) write_stats();
        } else if (bam_ && !closed_) {
            encode_buffer(true);
            buf_.append(reinterpret_cast<const char *>(kBgzfEof), sizeof kBgzfEof);
            join_writer();
            out_.write(buf_.data(), static_cast<std::streamsize>(buf_.size()));
            buf_.clear();
        } else if (!closed_) {
            flush();
        }
        closed_ = true;
        join_writer();
        out_.flush();
        if (!out_) throw std::runtime_error("writing the SAM file failed");
    }
    void header(const std::vector<std::string> &ref_ids, const std::vector<size_t> &ref_lengths) {
        buf_ += sorter_ ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\n";
        for (size_t i = 0; i < ref_ids.size(); i++) {
            buf_ += "@SQ\tSN:";
            buf_ += ref_ids[i];
            buf_ += "\tLN:";
            number(ref_lengths[i]);
            buf_ += '\n';
        }
        if (bam_) {                                   // the BAM header: blocks of its own, before any record
            std::string head;
            bam_header(buf_, ref_ids, ref_lengths, head, ref_index_);
            blocks_.clear();
            bam_->deflate(reinterpret_cast<const uint8_t *>(head.data()), head.size(), blocks_);
            join_writer();
            out_.write(reinterpret_cast<const char *>(blocks_.data()), static_cast<std::streamsize>(blocks_.size()));
            header_bytes_ = blocks_.size();
            n_ref_ = ref_ids.size();
            if (!depth_file_.empty() || !coverage_file_.empty()) {
                sorter_->set_depth(ref_lengths);
                ref_ids_ = ref_ids;
                ref_len_.assign(ref_lengths.begin(), ref_lengths.end());   // set_depth has refused what does not fit
            }
            if (pileup_on()) {
                set_pileup(ref_ids, ref_lengths);
                ref_ids_ = ref_ids;
            }
            if (!stats_file_.empty()) sorter_->set_stats(stats_params_);
            buf_.clear();
        }
    }
    // QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL [tags: "NM:i:3\tMD:Z:..." -- appended after a tab when not empty];
    // RNEXT PNEXT TLEN are * 0 0 for every record but those of --paired
    static void format(std::string &buf, std::string_view qname, unsigned flag, std::string_view rname, uint64_t pos, unsigned mapq,
                       std::string_view cigar, std::string_view seq, std::string_view qual, std::string_view tags = {},
                       std::string_view rnext = "*", uint64_t pnext = 0, int64_t tlen = 0) {
        buf.append(qname); buf += '\t';
        number(buf, flag); buf += '\t';
        buf.append(rname); buf += '\t';
        number(buf, pos); buf += '\t';
        number(buf, mapq); buf += '\t';
        buf.append(cigar); buf += '\t';
        buf.append(rnext); buf += '\t';
        number(buf, pnext); buf += '\t';
        if (tlen < 0) buf += '-';
        number(buf, tlen < 0 ? static_cast<uint64_t>(-tlen) : static_cast<uint64_t>(tlen)); buf += '\t';
        buf.append(seq); buf += '\t';
        buf.append(qual);
        if (!tags.empty()) {
            buf += '\t';
            buf.append(tags);
        }
        buf += '\n';
    }
    void record(std::string_view qname, unsigned flag, std::string_view rname, uint64_t pos, unsigned mapq, std::string_view cigar,
                std::string_view seq, std::string_view qual, std::string_view tags = {}, std::string_view rnext = "*", uint64_t pnext = 0,
                int64_t tlen = 0) {
        format(buf_, qname, flag, rname, pos, mapq, cigar, seq, qual, tags, rnext, pnext, tlen);
        if (buf_.size() > (4u << 20)) flush();
    }
    // records formatted elsewhere (format(): a few threads, each a block of reads), appended in order
    void append(std::string_view records) {
        buf_.append(records);
        if (buf_.size() > (4u << 20)) flush();
    }
};

class bucket_locator {
public:
    // (bucket id, offset in the bucket, window offset in the read, votes, true = read as-is)
    using locate_t = std::tuple<unsigned int, int, unsigned int, unsigned int, bool>;

private:
    mapper *_m;
    offset_scanner *_s;
    alignment_verifier *_v = nullptr;            // non-null: the BM_ALIGN behaviour
    block_compressor *_bam = nullptr;            // non-null: the output file is BAM, its BGZF blocks made by this
    size_t _sort_run_bytes = 0;                  // > 0: --sort, the BAM records in coordinate order with a .bai (host/bam_sort.h)
    bool _markdup = false;                       // --markdup: duplicates flagged 0x400 before the sort (include/bmd.h)
    std::filesystem::path _depth_file, _coverage_file;   // --depth / --coverage: the written records' depth and coverage (include/bmc.h)
    std::filesystem::path _pileup_file;          // --pileup: the variant sites of the written records (include/bmp.h)
    pileup_thresholds _pileup_thresholds{};
    std::filesystem::path _stats_file;           // --stats: the mapping statistics of the written records (include/bmq.h)
    stats_params _stats_params{};
    vcf_options _vcf{};                          // --vcf: the genotypes at the pileup's SNV sites (include/bmg.h)
    float _max_edit_rate = -1.f;                 // >= 0: the BM_ALIGN behaviour under an edit bound (--max-edit-rate)
    bool _annotate = false;                      // --annotate: forward-strand records with =/X CIGAR, NM and MD
    bool _clip = false;                          // --clip: those records with soft-clipped ends and AS, under these scores
    uint32_t _clip_match = 1, _clip_penalty = 2;
    bool _affine = false;                        // --affine: the written alignments realigned under affine gap costs, with AS
    affine_scores _affine_scores{};
    bool _left_align = false;                    // --left-align: the written alignments' indels at their leftmost forward place
    bool _clip_overlap = false;                  // --clip-overlap: the two records of a pair soft-clipped where they overlap
    uint64_t _overlap_pairs = 0, _overlap_cut = 0, _overlap_bases = 0;   // ... the pairs handed to the pass, cut, and the bases clipped
    bool _split = false;                         // --split: per read the non-conflicting clipped stretches of its candidates, a
    split_params _split_params{};                // primary and 0x800 supplementary records tied by SA:Z (the scores are --clip's)
    float _best_margin = -1.f;                   // >= 0: --best, one record per read; the margin is this rate x read length
    bool _paired = false;                        // --paired: records 2p and 2p + 1 of the FASTQ file are mates, placed together
    uint32_t _min_frag = 1, _max_frag = 1000;    // --frag-range: what a proper pair spans, leftmost to rightmost base
    bool _frag_auto = false;                     // --frag-auto: every verifier block learns the range from its own pairs
    uint32_t _frag_cap = 10000, _frag_min_pairs = 64;
    float _rescue_rate = -1.f;                   // >= 0: --rescue, a mate without a proper placement is sought beside its partner
    std::vector<uint8_t> flat_genome_;           // --annotate with a verifier that cannot annotate: the records back to back
    const Genome *genome_ = nullptr;
    std::vector<Bucket> buckets_;
    std::vector<uint64_t> bstart_;               // bucket views into the records laid back to back
    std::vector<uint32_t> blen_;

    unsigned int bucket_length, read_length, min_base_quality;
    uint8_t k;
    int allowed_mismatch, allowed_indel;
    float allowed_indel_rate;
    int num_samples;
    unsigned int num_segment_samples;

    // query_sequences_storage (:19-103), flat: window w of read r = first_window[r] + its rank among the
    // read's windows; samples are num_samples (hash, position) pairs per window.
    std::vector<uint32_t> first_window;          // per read (+1 sentinel)
    std::vector<int> window_start;               // per window: start inside the read
    std::vector<uint32_t> sample_hash;           // per window x num_samples
    std::vector<uint16_t> sample_pos;            // per window x num_samples
    std::vector<uint32_t> segment_length;        // per window
    std::vector<uint8_t> window_has_samples;     // windows shorter than k have none
    std::vector<unsigned int> read_lengths;      // per read

    static uint32_t kmer_hash_at(const char *s, uint32_t k_) {
        uint32_t h = 0;
        for (uint32_t t = 0; t < k_; t++) h = (h << 2) | dna4_rank(static_cast<uint8_t>(s[t]));
        return h;
    }

    uint32_t window_of(const segment_info_t &seg) const {
        for (uint32_t w = first_window[seg.first]; w < first_window[seg.first + 1]; w++)
            if (window_start[w] == seg.second) return w;
        throw std::runtime_error("the mapper returned a (read, window) pair the locator never sampled");
    }

    // _prepare_read_query (:292-347): the FASTQ pass and the windowing (:303-316) stay here; the sampling of
    // every window (:317-343) runs behind offset_scanner::sample_windows, a block of reads at a time.
    void prepare_read_query(const std::string &fastq) {
        first_window.clear(); window_start.clear(); sample_hash.clear(); sample_pos.clear();
        segment_length.clear(); window_has_samples.clear(); read_lengths.clear();
        std::vector<uint8_t> bases, quals;
        std::vector<uint64_t> win_start, qual_start;
        std::vector<uint32_t> win_len;
        const size_t block_bases = 256u << 20;
        // A regular file: nothing is copied here -- the windows are views into the mapped file (the index the mapper's pass
        // built, or is building), and the scanner gathers them where it needs them.
        if (std::shared_ptr<FastqFile> fq = FastqFile::open(fastq)) {
            const uint8_t *text = reinterpret_cast<const uint8_t *>(fq->data());
            size_t block = 0;
            auto flush_views = [&]() {
                const size_t n = win_start.size(), at = sample_hash.size();
                if (n == 0) return;
                sample_hash.resize(at + n * num_samples);
                sample_pos.resize(at + n * num_samples);
                const size_t has_at = window_has_samples.size();
                window_has_samples.resize(has_at + n);
                _s->sample_text_windows(text, fq->size(), win_start.data(), qual_start.data(), win_len.data(), static_cast<uint32_t>(n),
                                        min_base_quality, sample_hash.data() + at, sample_pos.data() + at, window_has_samples.data() + has_at);
                win_start.clear(); qual_start.clear(); win_len.clear();
                block = 0;
            };
            for (size_t i = 0;;) {
                const size_t n = fq->wait(i + 1);
                if (n <= i) break;
                for (; i < n; i++) {
                    const FastqFile::Rec &r = fq->rec(i);
                    const uint32_t len = r.len;
                    first_window.push_back(static_cast<uint32_t>(window_start.size()));
                    auto add = [&](uint32_t st) {
                        const uint32_t end = std::min(st + read_length, len);
                        window_start.push_back(static_cast<int>(st));
                        segment_length.push_back(end - st);
                        win_start.push_back(r.seq + st);
                        qual_start.push_back(r.qual + st);
                        win_len.push_back(end - st);
                    };
                    if (len > 2 * read_length)
                        for (uint32_t st : sample_deterministically(num_segment_samples, len - read_length - 1)) add(st);
                    else
                        add(0);
                    read_lengths.push_back(len);
                    block += len;
                    if (block >= block_bases) flush_views();
                }
            }
            flush_views();
            first_window.push_back(static_cast<uint32_t>(window_start.size()));
            return;
        }
        auto flush = [&]() {
            const size_t n = win_start.size(), at = sample_hash.size();
            if (n == 0) return;
            sample_hash.resize(at + n * num_samples);
            sample_pos.resize(at + n * num_samples);
            const size_t has_at = window_has_samples.size();
            window_has_samples.resize(has_at + n);
            _s->sample_windows(bases.data(), quals.data(), bases.size(), win_start.data(), win_len.data(),
                               static_cast<uint32_t>(n), min_base_quality, sample_hash.data() + at, sample_pos.data() + at,
                               window_has_samples.data() + has_at);
            bases.clear(); quals.clear(); win_start.clear(); win_len.clear();
        };
        for_each_fastq_stream(fastq, [&](const FastqRecord &rec) {
            const uint32_t len = static_cast<uint32_t>(rec.seq.size());
            first_window.push_back(static_cast<uint32_t>(window_start.size()));
            std::vector<uint32_t> starting_positions{0};
            if (len > 2 * read_length) starting_positions = sample_deterministically(num_segment_samples, len - read_length - 1);
            const uint64_t at = bases.size();
            bases.insert(bases.end(), rec.seq.begin(), rec.seq.end());
            quals.insert(quals.end(), rec.qual.begin(), rec.qual.end());
            for (uint32_t i : starting_positions) {
                const uint32_t end = std::min(i + read_length, len);
                window_start.push_back(static_cast<int>(i));
                segment_length.push_back(end - i);
                win_start.push_back(at + i);
                win_len.push_back(end - i);
            }
            read_lengths.push_back(len);
            if (bases.size() >= block_bases) flush();
        });
        flush();
        first_window.push_back(static_cast<uint32_t>(window_start.size()));
    }

    // _filter_best_locations (:350-405).  The reference keeps a std::map keyed (bucket, offset, strand); here the
    // proposals of a read live in one flat vector kept in that key order (a read has a handful of them):
    //   * an incoming location adds its votes to EVERY proposal of its bucket and strand whose offset lies in
    //     [offset - len * n, offset + len * n] -- float32 arithmetic, truncated towards zero (:365-366);
    //   * only when none took the votes does it become a proposal itself, with its own votes (:380);
    //   * all proposals holding the maximum come out, in key order (:390-402).
    // Pinned by tests/golden/sam_small.json (an independent plain-Python statement of the whole tool).
    struct proposal {
        unsigned int bucket;
        int offset;
        bool as_is;
        unsigned int votes;
        bool before(unsigned int b, int o, bool s) const {
            return std::tie(bucket, offset, as_is) < std::tie(b, o, s);
        }
    };
    std::vector<locate_t> filter_best_locations(const std::vector<locate_t> &mapped_locations, unsigned int read_len) const {
        std::vector<proposal> props;
        const float reach = read_len * allowed_indel_rate;
        for (const locate_t &loc : mapped_locations) {
            const unsigned int bucket = std::get<0>(loc), votes = std::get<3>(loc);
            const int offset = std::get<1>(loc);
            const bool as_is = std::get<4>(loc);
            const int lo = static_cast<int>(offset - reach), hi = static_cast<int>(offset + reach);
            bool taken = false;
            for (proposal &p : props)
                if (p.bucket == bucket && p.as_is == as_is && p.offset >= lo && p.offset <= hi) {
                    p.votes += votes;
                    taken = true;
                }
            if (taken) continue;
            auto at = std::find_if(props.begin(), props.end(), [&](const proposal &p) { return !p.before(bucket, offset, as_is); });
            props.insert(at, proposal{bucket, offset, as_is, votes});
        }
        unsigned int top = 0;
        for (const proposal &p : props) top = std::max(top, p.votes);
        std::vector<locate_t> best;
        for (const proposal &p : props)
            if (p.votes == top) best.emplace_back(p.bucket, p.offset, 0u, p.votes, p.as_is);
        return best;
    }

    // SEQ as seqan3 writes a dna4 vector: the reads were folded to A/C/G/T when they were parsed
    // (_phred94_traits, utils.h:192-204), so N / IUPAC / lower case never reach the SAM file.
    static void append_dna4(std::string &out, std::string_view seq) {
        static const std::array<char, 256> fold = [] {
            std::array<char, 256> t{};
            for (int c = 0; c < 256; c++) t[static_cast<size_t>(c)] = dna4_char(dna4_rank(static_cast<uint8_t>(c)));
            return t;
        }();
        const size_t at = out.size();
        out.resize(at + seq.size());
        for (size_t i = 0; i < seq.size(); i++) out[at + i] = fold[static_cast<uint8_t>(seq[i])];
    }

public:
    // bucket_locator ctor (:409-432); the indexer pointer of the reference is replaced by the genome
    // (locator::initialize -> indexer::index is done by the caller, see main.cpp).
    bucket_locator(mapper *map, offset_scanner *scanner, unsigned int bucket_len, unsigned int read_len,
                   uint8_t seed_len, float mismatch_rate, float indel_rate, unsigned int sample_size,
                   unsigned int quality_threshold, unsigned int num_segment_samples_ = 5)
        : _m(map), _s(scanner), bucket_length(bucket_len), read_length(read_len), k(seed_len) {
        allowed_mismatch = static_cast<int>(ceil_mul_f32(mismatch_rate, sample_size));   // :419
        allowed_indel = static_cast<int>(ceil_mul_f32(indel_rate, read_len));            // :420
        allowed_indel_rate = indel_rate;
        num_samples = static_cast<int>(sample_size);
        num_segment_samples = num_segment_samples_;
        min_base_quality = quality_threshold * k;                                         // :431
    }

    // bucketmap_align: every located candidate is verified by a pairwise alignment before it is written
    void set_verifier(alignment_verifier *v) { _v = v; }
    void set_compressor(block_compressor *c) { _bam = c; }   // the output file is BAM (-o x.bam)
    void set_sort(size_t run_bytes) { _sort_run_bytes = run_bytes; }   // ... coordinate-sorted, in runs of this many bytes
    void set_markdup(bool on) { _markdup = on; }                       // ... with its duplicates flagged
    void set_depth_files(std::filesystem::path const &depth, std::filesystem::path const &coverage) {   // ... and its depth reported
        _depth_file = depth;
        _coverage_file = coverage;
    }
    void set_pileup(std::filesystem::path const &file, pileup_thresholds const &th) {   // ... and its variant sites listed
        _pileup_file = file;
        _pileup_thresholds = th;
    }
    // --vcf: genotypes at the SNV sites of the pileup under th, which is counted whether set_pileup names a file or not
    void set_vcf(vcf_options const &vcf, pileup_thresholds const &th) {
        _vcf = vcf;
        _pileup_thresholds = th;
    }
    void set_stats(std::filesystem::path const &file, stats_params const &pr) {   // ... and its mapping statistics reported
        _stats_file = file;
        _stats_params = pr;
    }
    // --max-edit-rate R: write_verified keeps only alignments within (uint32_t)(R * read length) edits; negative = unset
    void set_max_edit_rate(float r) { _max_edit_rate = r; }
    // --annotate: write_verified writes every record on the forward strand (POS, SEQ, QUAL, =/X/I/D CIGAR) with NM and MD
    void set_annotate(bool on) { _annotate = on; }
    // --clip: the --annotate layout, the written alignments through the verifier's clipping pass instead (POS, CIGAR, NM and MD
    // of the kept part, S entries, AS:i); an alignment of which nothing is kept writes no record
    // --best: every read's candidates go through the verifier as one group (alignment_verifier::best), the read gets ONE record,
    // its best alignment's, with MAPQ and X0 from best_mapq.h; margin = max(1, (uint32_t)(rate x read length))
    void set_best(float margin_rate) { _best_margin = margin_rate; }
    // --paired: the FASTQ file is interleaved; the two mates' candidates go through the verifier together
    // (alignment_verifier::paired) and each mate gets the record of its PICK, with the pair's flags, RNEXT, PNEXT and TLEN and
    // the MAPQ and X0 of pair_mapq.h.  Implies --best (the caller sets its margin) and --annotate.
    void set_paired(uint32_t min_frag, uint32_t max_frag) {
        _paired = _annotate = true;
        if (_best_margin < 0.f) _best_margin = 0.05f;
        _min_frag = min_frag;
        _max_frag = max_frag;
    }
    // --frag-auto (implies --paired: the caller sets it): every verifier block learns its range from its own pairs
    // (alignment_verifier::paired_auto; spans up to cap, at least min_pairs informative pairs, else --frag-range's); the block's
    // range is what its rescue uses too, a block's result depends on nothing outside it, and every block says on stderr what it
    // applied
    void set_frag_auto(uint32_t cap, uint32_t min_pairs) {
        _frag_auto = true;
        _frag_cap = cap;
        _frag_min_pairs = min_pairs;
    }
    // --rescue (implies --paired: the caller sets it): after a block's paired() call every pair without a proper combination
    // gets the jobs of pair_rescue.h's select_rescue -- a mate's own winner within (uint32_t)(rate x its length) edits anchors
    // the search for the other mate (alignment_verifier::rescue) --, and a mate that comes back within bound and proper gets the
    // record of that placement, with its anchor's MAPQ, X0:i:1 and XR:i:1
    void set_rescue(float rate) { _rescue_rate = rate; }
    // --affine: the --annotate layout, the written alignments through the verifier's realignment pass first (POS, CIGAR, NM and
    // MD are the realigned path's; AS:i its affine score, unless --clip writes its own)
    void set_affine(const affine_scores &scores) {
        _affine = _annotate = true;
        _affine_scores = scores;
    }
    // --left-align: the --annotate layout, the written alignments through the verifier's normalisation pass (after the
    // realignment, before annotate or clip): POS, CIGAR, NM and MD are the normalised path's; with --affine and without --clip
    // AS:i is computed from the written entries (sam_tags::affine_score)
    void set_left_align() { _left_align = _annotate = true; }
    void set_clip(uint32_t match, uint32_t penalty) {
        _clip = _annotate = true;
        _clip_match = match;
        _clip_penalty = penalty;
    }
    // --clip-overlap (needs set_paired): the written alignments go through the verifier's overlap pass instead of annotate or clip --
    // under --clip with its scores, else without scores --, which soft-clips the two records of a pair that can carry 0x2 at one
    // cut where they overlap on the reference: POS, CIGAR, NM, MD, PNEXT (and AS:i) follow, TLEN stays, as the outer ends do
    void set_clip_overlap() { _clip_overlap = _annotate = true; }
    // --split: the --clip layout; of a read's candidates the verifier's split pass chooses the segments, only those go through
    // realign / left_align / clip, and they are written in chosen order: the first as the primary record, the others with flag
    // 0x800, MAPQ from split_mapq, and -- two or more -- each with an SA:Z tag naming the others (split_pick.h).  Needs set_clip.
    void set_split(uint32_t min_score, uint32_t max_overlap_permille, uint32_t max_segments) {
        _split = true;
        _split_params.min_score = min_score;
        _split_params.max_overlap_permille = max_overlap_permille;
        _split_params.max_segments = max_segments;
    }

    int get_allowed_mismatch() const { return allowed_mismatch; }
    int get_allowed_indel() const { return allowed_indel; }

    // initialize (:440-453): remember the genome, load the q-gram index into the mapper.
    // (Tried: the genome upload begun HERE, under the index load -- everything the locator needs was there no sooner, the
    // upload being the longest of the three passes either way, and map() took twice as long for sharing the link with it
    // from its first batch on: 0.09 -> 0.22 s per 1 M reads.  It starts with map(), in locate_reads.)
    void initialize(const Genome &genome, std::filesystem::path const &index_directory, std::string const &indicator) {
        genome_ = &genome;
        _m->load(index_directory, indicator);
    }

    ~bucket_locator() {
        if (uploader_.joinable()) uploader_.join();
    }

private:
    // BM_SERIAL_PASSES=1 (measurement): the upload and the sampling pass start when map() has returned, so that map()'s own
    // time can be read without two other passes sharing the PCIe link and the cores with it
    bool serial_passes_ = std::getenv("BM_SERIAL_PASSES") != nullptr;
    std::thread uploader_;
    std::exception_ptr upload_error_;
    float upload_ms_ = 0.f;
    bool upload_started_ = false;

    // the bucket sequences as views into one byte string that goes to the devices (_initialize_kmer_index, :151-160)
    void start_genome_upload() {
        if (upload_started_) return;
        upload_started_ = true;
        buckets_ = cut_buckets(*genome_, static_cast<int>(bucket_length), static_cast<int>(read_length));
        const auto t_begin = std::chrono::steady_clock::now();
        uploader_ = std::thread([this, t_begin]() {
            try {
                // the records go to the devices back to back, each from where it lies (no flattened copy on the host)
                const size_t n_rec = genome_->seqs.size();
                std::vector<uint64_t> rec_off(n_rec + 1, 0), rec_len(n_rec);
                std::vector<const uint8_t *> rec(n_rec);
                for (size_t r = 0; r < n_rec; r++) {
                    rec[r] = reinterpret_cast<const uint8_t *>(genome_->seqs[r].data());
                    rec_len[r] = genome_->seqs[r].size();
                    rec_off[r + 1] = rec_off[r] + rec_len[r];
                }
                bstart_.assign(buckets_.size(), 0);
                blen_.assign(buckets_.size(), 0);
                for (size_t b = 0; b < buckets_.size(); b++) {
                    bstart_[b] = rec_off[buckets_[b].record] + buckets_[b].start;
                    blen_[b] = buckets_[b].end - buckets_[b].start;
                }
                _s->load_genome_records(rec.data(), rec_len.data(), static_cast<uint32_t>(n_rec), bstart_.data(), blen_.data(),
                                        static_cast<uint32_t>(buckets_.size()));
                if (_v) _v->load_genome_records(rec.data(), rec_len.data(), static_cast<uint32_t>(n_rec));
            } catch (...) {
                upload_error_ = std::current_exception();
            }
            upload_ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        });
    }

public:
    // _locate (:613-705)
    std::vector<std::vector<locate_t>> locate_reads(const std::string &sequence_file) {
        // _initialize_kmer_index (:151-160: the bucket sequences to the devices) and _prepare_read_query (:292-347: the
        // locator's own pass over the FASTQ file) do not depend on the mapper's results, so each runs on a thread of its own
        // while _m->map() lays out the reads' windows and drives the filter.
        if (!serial_passes_) start_genome_upload();
        // (two threads: the upload touches the scanner's genome buffers, the sampling its window buffers and its stream)
        std::exception_ptr sampling_error;
        const auto t_side = std::chrono::steady_clock::now();
        float sampling_ms = 0.f;
        segments_t sequence_ids_orig, sequence_ids_rev_comp;
        if (serial_passes_) {
            std::tie(sequence_ids_orig, sequence_ids_rev_comp) = _m->map(sequence_file);
            _m->reset();
            start_genome_upload();
        }
        std::thread sampler([&]() {
            try {
                prepare_read_query(sequence_file);
            } catch (...) {
                sampling_error = std::current_exception();
            }
            sampling_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_side).count();
        });
        try {
            if (!serial_passes_) {
                std::tie(sequence_ids_orig, sequence_ids_rev_comp) = _m->map(sequence_file);
                _m->reset();
            }
        } catch (...) {
            if (uploader_.joinable()) uploader_.join();
            sampler.join();
            throw;
        }
        auto t0 = std::chrono::steady_clock::now();
        if (uploader_.joinable()) uploader_.join();
        sampler.join();
        upload_started_ = false;                                 // (a second locate() on this object uploads again)
        if (upload_error_) {
            std::exception_ptr e = upload_error_;
            upload_error_ = nullptr;
            std::rethrow_exception(e);
        }
        if (sampling_error) std::rethrow_exception(sampling_error);
        if (std::getenv("BM_LOG_BATCHES"))
            std::cerr << "[bm] beside map(): genome upload done after " << upload_ms_ << " ms, k-mer sampling pass after "
                      << sampling_ms << " ms, map() returned after " << std::chrono::duration<float, std::milli>(t0 - t_side).count()
                      << " ms, both passes and the upload done after "
                      << std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_side).count() << " ms\n";

        // Candidates in the order of the reference's bucket loop (:651-693): buckets ascending; inside a
        // bucket the reads as-is in list order, then the reverse complements in REVERSE list order.
        std::vector<uint32_t> pair_bucket, pair_window;
        std::vector<uint8_t> pair_rc;
        std::vector<segment_info_t> pair_seg;
        for (size_t i = 0; i < sequence_ids_orig.size(); i++) {
            if (i >= buckets_.size()) break;   // padding bucket ids (NB > kept buckets) hold no sequence
            auto push = [&](const segment_info_t &id, bool rc) {
                const uint32_t w = window_of(id);
                if (!window_has_samples[w]) return;
                pair_bucket.push_back(static_cast<uint32_t>(i));
                pair_window.push_back(w);
                pair_rc.push_back(rc ? 1 : 0);
                pair_seg.push_back(id);
            };
            for (auto &id : sequence_ids_orig[i]) push(id, false);
            auto &rev = sequence_ids_rev_comp[i];
            for (auto it = rev.rbegin(); it != rev.rend(); ++it) push(*it, true);
        }
        const float prep_s = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
        t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> offsets(pair_bucket.size());
        std::vector<uint32_t> votes(pair_bucket.size());
        if (!pair_bucket.empty())
            _s->scan(sample_hash.data(), sample_pos.data(), segment_length.data(), static_cast<uint32_t>(segment_length.size()),
                     pair_bucket.data(), pair_window.data(), pair_rc.data(), static_cast<uint32_t>(pair_bucket.size()),
                     offsets.data(), votes.data());
        const float scan_s = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();

        std::vector<std::vector<locate_t>> res(_m->num_records);
        for (size_t i = 0; i < pair_bucket.size(); i++) {
            const int offset = offsets[i];
            if (offset <= 0) continue;                                                      // :674,686
            const segment_info_t &id = pair_seg[i];
            if (!pair_rc[i]) {
                res[id.first].push_back(std::make_tuple(pair_bucket[i], offset - id.second,
                                                        static_cast<unsigned int>(id.second), votes[i], true));
            } else {
                // get_read_length / get_segment_length return uint16_t in the reference (:53-60)
                const int segment_offset_ = static_cast<uint16_t>(read_lengths[id.first]) - id.second -
                                            static_cast<uint16_t>(segment_length[pair_window[i]]);
                res[id.first].push_back(std::make_tuple(pair_bucket[i], offset - segment_offset_,
                                                        static_cast<unsigned int>(id.second), votes[i], false));
            }
        }
        // the reference times the per-bucket index build and the offset search separately; both are
        // one device pass here, reported under the second label
        std::cerr << "[BENCHMARK]\tTotal time used for building k-mer index for each bucket: " << prep_s << " s.\n";
        std::cerr << "[BENCHMARK]\tTotal time used for finding exact location of the sequences: " << scan_s << " s ("
                  << scan_s * 1000 * 1000 / _m->num_records << " μs/seq).\n";
        return res;
    }

    // .bucket_id -> @SQ lines and per-bucket offsets (:473-503).  One line per kept bucket; the reference name of
    // a bucket is its line up to the first blank, consecutive buckets of one name form one @SQ entry whose
    // length is the upper bound #buckets * bucket_len (:491,502) -- two FASTA records whose headers agree up to
    // the first blank therefore share an entry and the second one's offsets carry on from the first's.
    struct sam_header {
        std::vector<std::string> bucket_name, ref_ids;
        std::vector<unsigned int> bucket_offsets;
        std::vector<size_t> ref_lengths;
    };
    sam_header read_bucket_ids(std::filesystem::path const &index_file) const {
        sam_header h;
        std::ifstream in(index_file);
        std::string line;
        for (size_t b = 0; b < buckets_.size(); b++) {
            line.clear();
            std::getline(in, line);
            line.resize(std::min(line.size(), line.find(' ')));
            h.bucket_name.push_back(line);
        }
        // runs of equal consecutive names: one entry per run, offsets counted from the run's first bucket
        for (size_t b = 0, e = 0; b < h.bucket_name.size(); b = e) {
            for (e = b; e < h.bucket_name.size() && h.bucket_name[e] == h.bucket_name[b]; e++)
                h.bucket_offsets.push_back(static_cast<unsigned int>(e - b) * bucket_length);
            h.ref_ids.push_back(h.bucket_name[b]);
            h.ref_lengths.push_back((e - b) * static_cast<size_t>(bucket_length));
        }
        return h;
    }

    // locate (:455-611): one SAM record per surviving location.  Without a verifier this is the plain
    // `bucketmap` branch (best locations by votes, MAPQ from votes, no CIGAR); with one it is the BM_ALIGN
    // branch (every location aligned, MAPQ = 60 + score, dropped below `quality_threshold`, CIGAR written).
    void locate(const std::string &sequence_file, std::filesystem::path const &index_file,
                std::filesystem::path const &sam_file, unsigned int quality_threshold = 30) {
        auto locate_res = locate_reads(sequence_file);
        const sam_header h = read_bucket_ids(index_file);

        // --pileup: the bases of the header's references.  A reference is a run of kept buckets, bucket k of the run at
        // [k * bucket_length, (k + 1) * bucket_length): for one FASTA record that is the record itself, cut or filled up to whole
        // buckets; what no bucket's sequence fills has no reference allele (N).
        std::vector<std::string> pileup_bases;
        if ((!_pileup_file.empty() || _vcf.on()) && genome_) {
            for (size_t b = 0, r = 0; r < h.ref_ids.size(); r++) {
                pileup_bases.emplace_back(h.ref_lengths[r], 'N');
                for (size_t at = 0; at < h.ref_lengths[r]; at += bucket_length, b++) {
                    const std::string &seq = genome_->seqs[buckets_[b].record];
                    const size_t start = buckets_[b].start, n = std::min<size_t>(bucket_length, seq.size() - std::min<size_t>(start, seq.size()));
                    pileup_bases.back().replace(at, n, seq, start, n);
                }
            }
        }
        sam_text sam(sam_file, _bam, _sort_run_bytes, _markdup, _depth_file, _coverage_file, _pileup_file, _pileup_thresholds, &pileup_bases, _vcf);
        sam.set_stats(_stats_file, _stats_params);
        sam.header(h.ref_ids, h.ref_lengths);
        unsigned int read_id = 0, mapped_locations = 0;
        auto t0 = std::chrono::steady_clock::now();
        if (_v) {
            mapped_locations = write_verified(sequence_file, locate_res, h, sam, quality_threshold, read_id);
        } else if (std::shared_ptr<FastqFile> fq = FastqFile::open(sequence_file)) {
            // the records of a block of reads are formatted by a thread of their own (blocks of 16 384 reads, rounds of up to
            // eight) and appended in read order: formatting 640 MB of SAM text on one thread was the tool's longest stage
            const size_t n = fq->count(), block = 16384;
            const unsigned T = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
            std::vector<std::string> text(T);
            std::vector<unsigned int> made(T);
            auto format_block = [&](unsigned t, size_t r0, size_t r1) {
                std::string &out = text[t], seq;
                out.clear();
                made[t] = 0;
                for (size_t r = r0; r < r1; r++) {
                    const FastqRecord rec = fq->view(r);
                    auto best = filter_best_locations(locate_res[r], static_cast<unsigned int>(rec.seq.size()));   // :540
                    if (best.empty()) continue;
                    seq.clear();
                    append_dna4(seq, rec.seq);
                    for (auto &[bucket_id, offset, segment_offset, votes, is_original] : best) {
                        (void)segment_offset;
                        const unsigned int map_qual = std::min(60u, 6 * votes);                      // :591
                        const size_t ref_offset = static_cast<size_t>(h.bucket_offsets[bucket_id]) + offset;  // :592, 0-based
                        sam_text::format(out, rec.id, is_original ? 0 : 16, h.bucket_name[bucket_id], ref_offset + 1, map_qual, "*", seq, rec.qual);
                        made[t]++;
                    }
                }
            };
            for (size_t r0 = 0; r0 < n; r0 += T * block) {
                std::vector<std::thread> pool;
                unsigned used = 0;
                for (unsigned t = 0; t < T && r0 + t * block < n; t++, used++)
                    if (t) pool.emplace_back(format_block, t, r0 + t * block, std::min(n, r0 + (t + 1) * block));
                format_block(0, r0, std::min(n, r0 + block));
                for (auto &th : pool) th.join();
                for (unsigned t = 0; t < used; t++) {
                    sam.append(text[t]);
                    mapped_locations += made[t];
                }
            }
            read_id = static_cast<unsigned int>(n);
        } else {
            std::string seq;
            for_each_fastq_stream(sequence_file, [&](const FastqRecord &rec) {
                auto best = filter_best_locations(locate_res[read_id], static_cast<unsigned int>(rec.seq.size()));   // :540
                if (!best.empty()) {
                    seq.clear();
                    append_dna4(seq, rec.seq);
                }
                for (auto &[bucket_id, offset, segment_offset, votes, is_original] : best) {
                    (void)segment_offset;
                    const unsigned int map_qual = std::min(60u, 6 * votes);                      // :591
                    const size_t ref_offset = static_cast<size_t>(h.bucket_offsets[bucket_id]) + offset;  // :592, 0-based
                    sam.record(rec.id, is_original ? 0 : 16, h.bucket_name[bucket_id], ref_offset + 1, map_qual, "*", seq, rec.qual);
                    mapped_locations++;
                }
                read_id++;
            });
        }
        sam.close();                                             // (every record is in the file before the time is taken)
        const float s = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
        std::cerr << "[BENCHMARK]\tTotal mapped locations: " << mapped_locations << " ("
                  << static_cast<float>(mapped_locations) / read_id << " per sequence).\n";
        std::cerr << "[BENCHMARK]\tTotal time used for alignment verification and output: " << s << " s ("
                  << s / mapped_locations * 1000 * 1000 << " μs per pairwise alignment).\n";
    }

private:
    // BM_ALIGN branch of locate (:520-528,544-589), a block of reads at a time: the text window of every
    // location (:549-550), one batch of alignments, then the records in read order.
    //   * no _filter_best_locations in this branch (:538-541);
    //   * width = min(len + 1 + (size_t)(n * len), bucket size - offset), the product in float32 (:550);
    //   * map_qual = 60u + score in UNSIGNED arithmetic: below -60 it wraps to ~2^32 and so passes the
    //     `< quality_threshold` test (:570-573); the SAM field is 8 bits wide, hence the truncation;
    //   * POS = begin + bucket offset + offset + 1, also on the reverse strand, where `begin` counts in the
    //     reverse-complemented window (:576) -- kept as the reference computes it.  Flag-16 records therefore carry a POS
    //     counted from the wrong end of the window, the read as sequenced and a CIGAR in read direction: not usable SAM.
    // --annotate (set_annotate) is where the tool leaves that layout: the written alignments of a block go through the
    // verifier's annotation pass and their records become POS = bucket offset + clipped offset + forward pos + 1, the
    // =/X/I/D CIGAR along the forward strand, for flag 16 the reverse complement of the folded read and the reversed
    // qualities, and NM:i / MD:Z tags.  MAPQ, flags, RNAME, record order and which records exist stay as they are.
    // --clip (set_clip) sends them through the clipping pass instead: POS, CIGAR, NM and MD describe the kept part, the
    // clipped ends are S entries (SEQ and QUAL stay whole), AS:i carries the kept part's score, and an alignment of which
    // nothing is kept has no record.
    // Deviation: a negative `offset` indexes before the bucket in the reference (undefined behaviour); here
    // the window is clipped to start at the bucket's first base.
    unsigned int write_verified(const std::string &sequence_file, const std::vector<std::vector<locate_t>> &locate_res,
                                const sam_header &h, sam_text &sam, unsigned int quality_threshold, unsigned int &read_id) {
        // Two blocks of reads: while the verifier works on one (a thread of its own), the records of the one before are
        // written and the next is read from the file.
        struct held { std::string id, seq, qual; uint64_t start; };
        struct Block {
            std::vector<held> reads;
            std::vector<uint8_t> bases;
            std::vector<uint64_t> text_start, query_start, cigar_offset;
            std::vector<uint32_t> text_len, query_len, begin, cigar, max_edits;
            std::vector<uint32_t> group_offset{0}, margin, hint, winner, edits, end;    // --best: a group per read
            std::vector<uint32_t> contig, pick;                 // --paired: per alignment its @SQ entry; per read its pick
            uint32_t min_frag = 0, max_frag = 0;                // --paired: the range the block's pick was made under
            std::vector<uint8_t> proper;                        // ... and per pair (reads 2p, 2p + 1 of the block)
            std::vector<uint64_t> s1, s2;
            std::vector<uint32_t> rescued_at;                   // --rescue: per read the alignment (appended behind the groups') that
                                                                // places it beside its mate, kBeyond when it was not rescued
            std::vector<uint8_t> text_rc;
            std::vector<int32_t> score;
            std::vector<uint32_t> ann_slot;      // --annotate: per alignment its place in `ann`, ~0u = not written
            clipping ann;                        // (--clip fills score and the clips too)
            std::vector<int32_t> affine_score;   // --affine: per slot of `ann` the realigned path's score
            std::vector<uint32_t> cut;           // --clip-overlap: per slot of `ann` the query bases the cut clipped
            split_result split;                  // --split: the verifier's answer for the block, a group per read ...
            std::vector<uint8_t> chosen;         // ... and per alignment whether it is one of its read's segments
            unsigned int first_read = 0;
            std::exception_ptr failed;
        } blocks[2];
        unsigned int mapped_locations = 0;
        size_t block_reads = 1u << 17;
        const size_t block_bases = 64u << 20;
        if (const char *e = std::getenv("BM_VERIFY_BLOCK_READS")) block_reads = std::max<size_t>(1, std::strtoull(e, nullptr, 10));   // tests
        int cur = 0, in_flight = -1, to_write = -1;
        blocks[0].first_read = read_id;
        std::thread worker;
        const bool bounded = _max_edit_rate >= 0.f;             // --max-edit-rate: rejected alignments leave no record
        const bool best = _best_margin >= 0.f;                  // --best: neither do the alignments that did not win
        const bool paired = _paired;                            // --paired: --best with the pick of the pair in the winner's place
        const bool rescue = paired && _rescue_rate >= 0.f;      // --rescue: pairs without a proper combination get a second look
        std::vector<uint32_t> bucket_ref;                       // per bucket the index of its @SQ entry (runs of equal names)
        const bool split = _split;                              // --split: the chosen segments of a read, and only they
        if (split && !_clip) throw std::runtime_error("--split writes --clip's records: set_clip comes first");
        if (split)
            for (size_t bk = 0; bk < h.bucket_name.size(); bk++)
                bucket_ref.push_back(bk == 0 ? 0u : bucket_ref[bk - 1] + (h.bucket_name[bk] == h.bucket_name[bk - 1] ? 0u : 1u));
        if (paired) {
            if (locate_res.size() % 2u)
                throw std::runtime_error(sequence_file + " holds " + std::to_string(locate_res.size()) +
                                         " records, an odd number: --paired takes one interleaved FASTQ file, records 2p and 2p + 1 being mates");
            for (size_t bk = 0; bk < h.bucket_name.size(); bk++)
                bucket_ref.push_back(bk == 0 ? 0u : bucket_ref[bk - 1] + (h.bucket_name[bk] == h.bucket_name[bk - 1] ? 0u : 1u));
        }
        // --annotate with a verifier that has no annotation pass (the oracle-backed test tools): sam_tags::annotate_on_host
        const bool annotate_here = _annotate && !_clip && !_clip_overlap && !_v->can_annotate();
        if (_clip_overlap && !paired) throw std::runtime_error("--clip-overlap clips the mates of pairs: set_paired comes first");
        if ((annotate_here || (_affine && !_v->can_realign()) || (_left_align && !_v->can_left_align()) ||
             (_clip_overlap && !_v->can_clip_overlap())) && flat_genome_.empty())
            for (const auto &seq : genome_->seqs) flat_genome_.insert(flat_genome_.end(), seq.begin(), seq.end());
        auto is_written = [&](const Block &b, size_t a) {       // :570-573, and the edit bound
            if (split) return b.chosen[a] != 0;                 // (--split: 60 + score means nothing for a part of a read)
            const size_t map_qual = 60u + static_cast<unsigned int>(b.score[a]);
            return !((bounded || best) && b.score[a] == alignment_verifier::kRejected) && !(map_qual < quality_threshold);
        };
        // --clip: the kept range of written alignment a is empty.  A kept column scores at least `match`, so bmv_clip's score tells;
        // after --clip-overlap's cut a kept range may score 0 or less, but it holds a reference base
        auto nothing_kept = [&](const Block &b, size_t a) {
            const uint32_t s = b.ann_slot[a];
            return _clip_overlap ? b.ann.ref_len[s] == 0 : b.ann.score[s] == 0;
        };
        // --rescue, after paired(): the jobs of every pair that is not proper, the verifier's answer, and for each mate it
        // places a full alignment appended behind the groups' -- on its view narrowed to the m + d columns before the end the
        // rescue found, which yields the alignment the whole view would
        auto rescue_block = [&](Block &b) {
            const uint32_t kNone = alignment_verifier::kBeyond;
            struct job { uint32_t anchor_read, query_read, pair, which; };
            std::vector<job> jobs;
            std::vector<uint64_t> a_ts, c0, c1, qs;
            std::vector<uint32_t> a_tl, a_ql, a_end, ql, me;
            std::vector<uint8_t> a_rc;
            auto anchor_edits = [&](size_t r) { return b.winner[r] == kNone ? kNone : b.edits[b.winner[r]]; };
            for (size_t p = 0; p < b.reads.size() / 2; p++) {
                const uint32_t edits[2] = {anchor_edits(2 * p), anchor_edits(2 * p + 1)};
                const uint32_t len[2] = {static_cast<uint32_t>(b.reads[2 * p].seq.size()), static_cast<uint32_t>(b.reads[2 * p + 1].seq.size())};
                const rescue_choice c = select_rescue(b.proper[p] != 0, edits, len, _rescue_rate, nullptr, nullptr);
                for (uint32_t i = 0; i < 2u; i++) {
                    if (!c.job[i]) continue;
                    const uint32_t ra = static_cast<uint32_t>(2 * p + i), rq = static_cast<uint32_t>(2 * p + 1 - i), a = b.winner[ra];
                    const unsigned int bucket = std::get<0>(locate_res[b.first_read + ra][a - b.group_offset[ra]]);
                    const uint64_t rec_start = bstart_[bucket] - buckets_[bucket].start;
                    jobs.push_back({ra, rq, static_cast<uint32_t>(p), i});
                    a_ts.push_back(b.text_start[a]); a_tl.push_back(b.text_len[a]); a_rc.push_back(b.text_rc[a]);
                    a_ql.push_back(b.query_len[a]); a_end.push_back(b.end[a]);
                    c0.push_back(rec_start); c1.push_back(rec_start + genome_->seqs[buckets_[bucket].record].size());
                    qs.push_back(b.reads[rq].start); ql.push_back(len[1 - i]); me.push_back(c.max_edits[i]);
                }
            }
            if (jobs.empty()) return;
            alignment_verifier::rescued out;
            _v->rescue(b.bases.data(), b.bases.size(), a_ts.data(), a_tl.data(), a_rc.data(), a_ql.data(), a_end.data(), c0.data(), c1.data(),
                       qs.data(), ql.data(), me.data(), static_cast<uint32_t>(jobs.size()), b.min_frag, b.max_frag, out);
            // per pair the job it keeps; its mate's placement, narrowed
            std::vector<uint64_t> ts, nqs;
            std::vector<uint32_t> tl, nql, readers;
            std::vector<uint8_t> trc;
            for (size_t j = 0; j < jobs.size();) {
                size_t e = j;
                uint32_t r_edits[2] = {kNone, kNone}, at[2] = {0, 0};
                uint8_t r_proper[2] = {0, 0};
                for (; e < jobs.size() && jobs[e].pair == jobs[j].pair; e++) {
                    r_edits[jobs[e].which] = out.edits[e];
                    r_proper[jobs[e].which] = out.proper[e];
                    at[jobs[e].which] = static_cast<uint32_t>(e);
                }
                const size_t p = jobs[j].pair;
                const uint32_t edits[2] = {anchor_edits(2 * p), anchor_edits(2 * p + 1)};
                const uint32_t len[2] = {static_cast<uint32_t>(b.reads[2 * p].seq.size()), static_cast<uint32_t>(b.reads[2 * p + 1].seq.size())};
                const rescue_choice c = select_rescue(false, edits, len, _rescue_rate, r_edits, r_proper);
                j = e;
                if (c.keep < 0) continue;
                const uint32_t k = at[c.keep], rq = jobs[k].query_read;
                const uint32_t span = std::min<uint64_t>(static_cast<uint64_t>(ql[k]) + out.edits[k], out.end[k]);
                ts.push_back(out.text_rc[k] ? out.text_start[k] + out.text_len[k] - out.end[k] : out.text_start[k] + out.end[k] - span);
                tl.push_back(span); trc.push_back(out.text_rc[k]);
                nqs.push_back(qs[k]); nql.push_back(ql[k]); readers.push_back(rq);
            }
            if (readers.empty()) return;
            std::vector<int32_t> score;
            std::vector<uint32_t> begin, cigar;
            std::vector<uint64_t> cigar_offset;
            _v->align(b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), nqs.data(), nql.data(), static_cast<uint32_t>(readers.size()),
                      score, begin, cigar_offset, cigar);
            for (size_t x = 0; x < readers.size(); x++) {
                const uint32_t rq = readers[x];
                // the mate's former winner, if it had one, gets no record
                if (b.pick[rq] != kNone) b.score[b.pick[rq]] = alignment_verifier::kRejected;
                b.rescued_at[rq] = static_cast<uint32_t>(b.text_start.size());
                b.text_start.push_back(ts[x]); b.text_len.push_back(tl[x]); b.text_rc.push_back(trc[x]);
                b.query_start.push_back(nqs[x]); b.query_len.push_back(nql[x]);
                const bool beyond = bounded && -static_cast<int64_t>(score[x]) >
                                                   static_cast<int64_t>(std::min(_max_edit_rate * static_cast<float>(nql[x]), 4e9f));
                b.score.push_back(beyond ? alignment_verifier::kRejected : score[x]);
                b.begin.push_back(begin[x]);
                b.cigar.insert(b.cigar.end(), cigar.begin() + static_cast<ptrdiff_t>(cigar_offset[x]),
                               cigar.begin() + static_cast<ptrdiff_t>(cigar_offset[x + 1]));
                b.cigar_offset.push_back(b.cigar.size());
            }
        };
        auto align = [&](Block &b) {                            // on the worker thread
            try {
                b.rescued_at.assign(b.reads.size(), alignment_verifier::kBeyond);
                b.min_frag = _min_frag;
                b.max_frag = _max_frag;
                if (paired && _frag_auto && !b.reads.empty()) {
                    alignment_verifier::frag_learned fl;
                    fl.applied_min = _min_frag;
                    fl.applied_max = _max_frag;
                    if (!b.text_start.empty())
                        _v->paired_auto(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(),
                                        b.query_start.data(), b.query_len.data(), static_cast<uint32_t>(b.text_start.size()),
                                        b.group_offset.data(), static_cast<uint32_t>(b.margin.size()), b.margin.data(), b.hint.data(),
                                        b.contig.data(), _frag_cap, _frag_min_pairs, _min_frag, _max_frag, b.score, b.begin, b.cigar_offset,
                                        b.cigar, b.winner, b.edits, b.end, b.pick, b.proper, b.s1, b.s2, fl);
                    b.min_frag = fl.applied_min;
                    b.max_frag = fl.applied_max;
                    std::string line = "[INFO]\tfragment range: " + std::to_string(fl.applied_min) + "," + std::to_string(fl.applied_max);
                    const std::string of = std::to_string(fl.n_informative) + " of " + std::to_string(b.reads.size() / 2);
                    if (fl.learned)
                        line += " learned from " + of + " pairs (quartiles " + std::to_string(fl.quartiles[0]) + " " +
                                std::to_string(fl.quartiles[1]) + " " + std::to_string(fl.quartiles[2]) + ")\n";
                    else
                        line += " kept, " + of + " pairs informative\n";
                    std::cerr << line;
                } else if (!b.text_start.empty() && paired)
                    _v->paired(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(),
                               b.query_start.data(), b.query_len.data(), static_cast<uint32_t>(b.text_start.size()), b.group_offset.data(),
                               static_cast<uint32_t>(b.margin.size()), b.margin.data(), b.hint.data(), b.contig.data(), _min_frag, _max_frag,
                               b.score, b.begin, b.cigar_offset, b.cigar, b.winner, b.edits, b.end, b.pick, b.proper, b.s1, b.s2);
                if (!b.text_start.empty() && paired) {
                    for (size_t a = 0; bounded && a < b.score.size(); a++)
                        if (b.score[a] != alignment_verifier::kRejected && -static_cast<int64_t>(b.score[a]) > static_cast<int64_t>(b.max_edits[a]))
                            b.score[a] = alignment_verifier::kRejected;
                    if (rescue) rescue_block(b);
                } else if (!b.text_start.empty() && best) {
                    _v->best(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(),
                             b.query_start.data(), b.query_len.data(), static_cast<uint32_t>(b.text_start.size()), b.group_offset.data(),
                             static_cast<uint32_t>(b.margin.size()), b.margin.data(), b.hint.data(), b.score, b.begin, b.cigar_offset,
                             b.cigar, b.winner, b.edits, b.end);
                    // --max-edit-rate on top: a winner beyond its bound leaves no record
                    for (size_t a = 0; bounded && a < b.score.size(); a++)
                        if (b.score[a] != alignment_verifier::kRejected && -static_cast<int64_t>(b.score[a]) > static_cast<int64_t>(b.max_edits[a]))
                            b.score[a] = alignment_verifier::kRejected;
                } else if (!b.text_start.empty() && bounded)
                    _v->align_bounded(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(),
                                      b.query_start.data(), b.query_len.data(), b.max_edits.data(),
                                      static_cast<uint32_t>(b.text_start.size()), b.score, b.begin, b.cigar_offset, b.cigar);
                else if (!b.text_start.empty())
                    _v->align(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(),
                              b.query_start.data(), b.query_len.data(), static_cast<uint32_t>(b.text_start.size()), b.score, b.begin,
                              b.cigar_offset, b.cigar);
                if (split) {                                    // every candidate's range and the pick, a group per read
                    const uint32_t n_groups = static_cast<uint32_t>(b.reads.size());
                    split_params sp = _split_params;
                    sp.match = _clip_match;
                    sp.penalty = _clip_penalty;
                    b.chosen.assign(b.text_start.size(), 0);
                    b.split.n_seg.assign(n_groups, 0);
                    if (!b.text_start.empty()) {
                        _v->split(b.bases.data(), b.bases.size(), b.text_start.data(), b.text_len.data(), b.text_rc.data(), b.query_start.data(),
                                  b.query_len.data(), b.begin.data(), b.cigar_offset.data(), b.cigar.data(), b.contig.data(),
                                  static_cast<uint32_t>(b.text_start.size()), b.group_offset.data(), n_groups, sp, b.split);
                        for (const uint32_t a : b.split.seg)
                            if (a != kSplitBeyond) b.chosen[a] = 1;
                    }
                }
                if (_annotate && !b.text_start.empty()) {       // the alignments that will be written, as a batch of their own
                    const size_t n = b.text_start.size();
                    std::vector<uint64_t> ts, qs, co{0};
                    std::vector<uint32_t> tl, ql, bg, cg;
                    std::vector<uint8_t> trc;
                    b.ann_slot.assign(n, ~0u);
                    for (size_t a = 0; a < n; a++) {
                        if (!is_written(b, a)) continue;
                        b.ann_slot[a] = static_cast<uint32_t>(ts.size());
                        ts.push_back(b.text_start[a]); tl.push_back(b.text_len[a]); trc.push_back(b.text_rc[a]);
                        qs.push_back(b.query_start[a]); ql.push_back(b.query_len[a]); bg.push_back(b.begin[a]);
                        cg.insert(cg.end(), b.cigar.begin() + static_cast<ptrdiff_t>(b.cigar_offset[a]),
                                  b.cigar.begin() + static_cast<ptrdiff_t>(b.cigar_offset[a + 1]));
                        co.push_back(cg.size());
                    }
                    if (_affine) {                              // the realigned begin and entries take the edit path's place
                        realignment ra;
                        _v->realign(flat_genome_.data(), b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), qs.data(), ql.data(),
                                    bg.data(), co.data(), cg.data(), static_cast<uint32_t>(ts.size()), _affine_scores, ra);
                        bg.swap(ra.begin);
                        co.swap(ra.cigar_offset);
                        cg.swap(ra.cigar);
                        b.affine_score.swap(ra.score);
                    }
                    if (_left_align) {                          // ... and the normalised ones theirs
                        left_alignment la;
                        _v->left_align(flat_genome_.data(), b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), qs.data(),
                                       ql.data(), bg.data(), co.data(), cg.data(), static_cast<uint32_t>(ts.size()), la);
                        bg.swap(la.begin);
                        co.swap(la.cigar_offset);
                        cg.swap(la.cigar);
                    }
                    if (_clip_overlap) {
                        // the two records of every pair that can carry 0x2 name each other: the picks of a proper pair, a rescued
                        // mate and its anchor.  A rescued alignment lies on its anchor's contig.
                        const uint32_t kNone = alignment_verifier::kBeyond;
                        std::vector<uint32_t> mate(ts.size(), overlap::kNoMate), ct(ts.size(), 0);
                        auto record_of = [&](size_t r) {        // the alignment read r's record is written from, or kNone
                            if (b.rescued_at[r] != kNone) return b.rescued_at[r];
                            return b.group_offset[r + 1] == b.group_offset[r] ? kNone : b.pick[r];
                        };
                        for (size_t a = 0; a < n && a < b.contig.size(); a++)
                            if (b.ann_slot[a] != ~0u) ct[b.ann_slot[a]] = b.contig[a];
                        uint64_t handed = 0;
                        for (size_t p = 0; p < b.reads.size() / 2; p++) {
                            const bool rescued = b.rescued_at[2 * p] != kNone || b.rescued_at[2 * p + 1] != kNone;
                            for (size_t r = 2 * p; rescued && r < 2 * p + 2; r++)
                                if (b.rescued_at[r] != kNone && b.ann_slot[b.rescued_at[r]] != ~0u && b.winner[r ^ 1u] != kNone)
                                    ct[b.ann_slot[b.rescued_at[r]]] = b.contig[b.winner[r ^ 1u]];
                            if (!rescued && !(p < b.proper.size() && b.proper[p] != 0)) continue;
                            const uint32_t a0 = record_of(2 * p), a1 = record_of(2 * p + 1);
                            if (a0 == kNone || a1 == kNone || b.ann_slot[a0] == ~0u || b.ann_slot[a1] == ~0u) continue;
                            mate[b.ann_slot[a0]] = b.ann_slot[a1];
                            mate[b.ann_slot[a1]] = b.ann_slot[a0];
                            handed++;
                        }
                        uint64_t pairs_cut = 0, bases_cut = 0;
                        _v->clip_overlap(flat_genome_.data(), b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), qs.data(),
                                         ql.data(), bg.data(), co.data(), cg.data(), mate.data(), ct.data(), static_cast<uint32_t>(ts.size()),
                                         _clip ? _clip_match : 0u, _clip ? _clip_penalty : 0u, b.ann, b.cut, pairs_cut, bases_cut);
                        _overlap_pairs += handed;
                        _overlap_cut += pairs_cut;
                        _overlap_bases += bases_cut;
                    } else if (_clip)
                        _v->clip(b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), qs.data(), ql.data(), bg.data(),
                                 co.data(), cg.data(), static_cast<uint32_t>(ts.size()), _clip_match, _clip_penalty, b.ann);
                    else if (annotate_here)
                        sam_tags::annotate_on_host(flat_genome_.data(), b.bases.data(), ts.data(), tl.data(), trc.data(), qs.data(), ql.data(),
                                                   bg.data(), co.data(), cg.data(), static_cast<uint32_t>(ts.size()), b.ann);
                    else
                        _v->annotate(b.bases.data(), b.bases.size(), ts.data(), tl.data(), trc.data(), qs.data(), ql.data(), bg.data(),
                                     co.data(), cg.data(), static_cast<uint32_t>(ts.size()), b.ann);
                }
            } catch (...) {
                b.failed = std::current_exception();
            }
        };
        // BM_DUMP_ALIGNMENTS=<file> (tests): every alignment the verifier returned, kept or not, one line each --
        // read, text start in the concatenated genome, text length, strand, query length, score, begin, CIGAR
        // (--best: the winners only)
        std::ofstream dump;
        if (const char *e = std::getenv("BM_DUMP_ALIGNMENTS")) dump.open(e);
        // --paired: the one record read r of the block may get -- its pick's, when it passes what a --best record passes
        struct mate_record {
            bool has = false, rc = false;
            unsigned int bucket = 0;
            uint64_t pos = 0;                                   // 1-based, as written
            uint32_t ref_len = 0;
        };
        // --rescue: where a rescued mate's view begins, as (bucket, offset in it): the bucket of the anchor's record that holds it
        auto rescued_place = [&](const Block &b, size_t r) {
            const size_t ra = r ^ 1u;
            unsigned int bucket = std::get<0>(locate_res[b.first_read + ra][b.winner[ra] - b.group_offset[ra]]);
            const uint32_t record = buckets_[bucket].record;
            const uint64_t local = b.text_start[b.rescued_at[r]] - (bstart_[bucket] - buckets_[bucket].start);
            while (bucket + 1u < buckets_.size() && buckets_[bucket + 1u].record == record && buckets_[bucket + 1u].start <= local) bucket++;
            while (bucket > 0u && buckets_[bucket - 1u].record == record && buckets_[bucket].start > local) bucket--;
            return std::make_pair(bucket, local - buckets_[bucket].start);
        };
        auto mate_of = [&](const Block &b, size_t r) {
            mate_record m;
            if (rescue && b.rescued_at[r] != alignment_verifier::kBeyond) {
                const uint32_t a = b.rescued_at[r];
                if (!is_written(b, a) || (_clip && nothing_kept(b, a))) return m;
                const auto [bucket, offset] = rescued_place(b, r);
                m.has = true;
                m.rc = b.text_rc[a] != 0;
                m.bucket = bucket;
                m.pos = static_cast<uint64_t>(b.ann.pos[b.ann_slot[a]]) + h.bucket_offsets[bucket] + offset + 1u;
                m.ref_len = b.ann.ref_len[b.ann_slot[a]];
                return m;
            }
            const uint32_t a0 = b.group_offset[r];
            if (b.group_offset[r + 1] == a0 || b.pick[r] == alignment_verifier::kBeyond) return m;
            const uint32_t a = b.pick[r];
            if (!is_written(b, a) || (_clip && nothing_kept(b, a))) return m;
            const locate_t &loc = locate_res[b.first_read + r][a - a0];
            const int offset = std::get<1>(loc);
            m.has = true;
            m.rc = !std::get<4>(loc);
            m.bucket = std::get<0>(loc);
            m.pos = static_cast<uint64_t>(b.ann.pos[b.ann_slot[a]]) + h.bucket_offsets[m.bucket] + (offset < 0 ? 0 : offset) + 1u;
            m.ref_len = b.ann.ref_len[b.ann_slot[a]];
            return m;
        };
        auto write = [&](Block &b) {
            if (b.failed) std::rethrow_exception(b.failed);
            size_t a = 0;
            std::string cg, tags, rc_seq, rc_qual, best_tag;
            // an annotated record of read r: alignment a, which begins ref_base bases into the @SQ entry rname
            auto annotated = [&](size_t r, size_t a, std::string_view rname, size_t ref_base, bool is_original, unsigned int flags,
                                 size_t map_qual, std::string_view last_tag, std::string_view rnext, uint64_t pnext, int64_t tlen) {
                const uint32_t s = b.ann_slot[a];
                const size_t ref_offset = static_cast<size_t>(b.ann.pos[s]) + ref_base;
                const uint32_t *entry = b.ann.xcigar.data() + b.ann.xcigar_offset[s];
                const size_t n_entries = b.ann.xcigar_offset[s + 1] - b.ann.xcigar_offset[s];
                cg.clear();
                sam_tags::append_cigar(cg, entry, n_entries);
                if (cg.empty()) cg = "*";
                tags = "NM:i:";
                sam_tags::number(tags, b.ann.nm[s]);
                tags += "\tMD:Z:";
                sam_tags::append_md(tags, entry, n_entries, b.ann.ref_bases.data() + b.ann.ref_offset[s]);
                if (_clip) {
                    tags += b.ann.score[s] < 0 ? "\tAS:i:-" : "\tAS:i:";   // (below 0 only after --clip-overlap's cut)
                    sam_tags::number(tags, static_cast<uint64_t>(std::abs(b.ann.score[s])));
                } else if (_affine) {                           // (--left-align: merges and drops change the score)
                    const int64_t as = _left_align || (_clip_overlap && b.cut[s] > 0)
                                           ? sam_tags::affine_score(entry, n_entries, _affine_scores.match, _affine_scores.mismatch,
                                                                            _affine_scores.gap_open, _affine_scores.gap_extend)
                                           : static_cast<int64_t>(b.affine_score[s]);
                    tags += as < 0 ? "\tAS:i:-" : "\tAS:i:";
                    sam_tags::number(tags, static_cast<uint64_t>(std::abs(as)));
                }
                if (best) tags += "\t" + best_tag;
                if (!last_tag.empty()) {
                    tags += '\t';
                    tags += last_tag;
                }
                if (!is_original && rc_seq.empty()) {
                    sam_tags::append_revcomp(rc_seq, b.reads[r].seq);
                    rc_qual.assign(b.reads[r].qual.rbegin(), b.reads[r].qual.rend());
                }
                sam.record(b.reads[r].id, (is_original ? 0 : 16) | flags, rname, ref_offset + 1, static_cast<uint8_t>(map_qual), cg,
                           is_original ? b.reads[r].seq : rc_seq, is_original ? b.reads[r].qual : rc_qual, tags, rnext, pnext, tlen);
                mapped_locations++;
            };
            auto own_quality = [&](size_t r) {                  // best_mapq of read r's own winner
                const uint32_t a0 = b.group_offset[r];
                return best_mapq(b.winner[r] - a0, b.edits.data() + a0, b.end.data() + a0, b.text_start.data() + a0, b.text_len.data() + a0,
                                 b.text_rc.data() + a0, b.group_offset[r + 1] - a0, b.margin[r]);
            };
            for (size_t r = 0; r < b.reads.size(); r++) {
                rc_seq.clear();                                 // (--annotate: made for the read's first flag-16 record)
                best_quality bq{0u, 0u};                        // --best: the MAPQ and X0 of the read's one record
                const bool candidates = best && b.group_offset[r + 1] > b.group_offset[r];
                const bool proper = paired && candidates && b.proper[r / 2] != 0;
                // --rescue: this read was placed beside its mate / its mate was placed beside this read
                const bool rescued = rescue && b.rescued_at[r] != alignment_verifier::kBeyond;
                const bool anchors = rescue && b.rescued_at[r ^ 1u] != alignment_verifier::kBeyond;
                if (proper) {
                    const uint32_t a0 = b.group_offset[r];
                    const size_t p = r / 2;
                    bq = pair_mate_mapq(pair_quality(b.s1[p], b.s2[p], static_cast<uint64_t>(b.margin[2 * p]) + b.margin[2 * p + 1]),
                                        b.pick[r] - a0, b.winner[r] - a0, b.edits.data() + a0, b.end.data() + a0, b.text_start.data() + a0,
                                        b.text_len.data() + a0, b.text_rc.data() + a0, b.group_offset[r + 1] - a0, b.margin[r]);
                } else if (rescued) {
                    bq = {own_quality(r ^ 1u).mapq, 1u};        // its place is only as unique as its anchor's
                } else if (candidates) {
                    bq = own_quality(r);
                }
                if (candidates || rescued) {
                    best_tag = "X0:i:";
                    sam_tags::number(best_tag, bq.x0);
                }
                // --paired: what the record says about the pair and about the mate's record
                unsigned int pair_flags = 0;
                std::string_view rnext = "*";
                uint64_t pnext = 0;
                int64_t tlen = 0;
                if (paired && (candidates || rescued)) {
                    const mate_record me = mate_of(b, r), mate = mate_of(b, r ^ 1u);
                    pair_flags = 0x1u | (r % 2 ? 0x80u : 0x40u);
                    if (!mate.has) {
                        pair_flags |= 0x8u;
                    } else {
                        if (proper || ((rescued || anchors) && me.has)) pair_flags |= 0x2u;
                        if (mate.rc) pair_flags |= 0x20u;
                        const bool same = bucket_ref[me.bucket] == bucket_ref[mate.bucket];
                        rnext = same ? std::string_view("=") : std::string_view(h.bucket_name[mate.bucket]);
                        pnext = mate.pos;
                        if (same && me.has) {
                            const uint64_t lo = std::min(me.pos, mate.pos), hi = std::max(me.pos + me.ref_len, mate.pos + mate.ref_len);
                            const bool leftmost = me.pos < mate.pos || (me.pos == mate.pos && r % 2 == 0);
                            tlen = leftmost ? static_cast<int64_t>(hi - lo) : -static_cast<int64_t>(hi - lo);
                        }
                    }
                }
                const uint32_t chosen = !candidates ? alignment_verifier::kBeyond : paired ? b.pick[r] : b.winner[r];
                for (auto &[bucket_id, offset, segment_offset, votes, is_original] : locate_res[b.first_read + r]) {
                    (void)segment_offset; (void)votes;
                    if (dump.is_open() && !(best && chosen != a)) {
                        dump << b.first_read + r << ' ' << b.text_start[a] << ' ' << b.text_len[a] << ' ' << int(b.text_rc[a]) << ' '
                             << b.query_len[a] << ' ' << b.score[a] << ' ' << b.begin[a] << ' ';
                        for (uint64_t x = b.cigar_offset[a]; x < b.cigar_offset[a + 1]; x++) dump << (b.cigar[x] >> 4) << "MID"[b.cigar[x] & 15u];
                        dump << (b.cigar_offset[a] == b.cigar_offset[a + 1] ? "*\n" : "\n");
                    }
                    if (split) {                                // (the read's records follow the loop, in chosen order)
                        a++;
                        continue;
                    }
                    const unsigned int wrapped = 60u + static_cast<unsigned int>(b.score[a]);        // :570
                    const size_t map_qual = best ? bq.mapq : wrapped;
                    if (is_written(b, a) && _clip && nothing_kept(b, a)) {
                        // --clip: the kept range is empty (a kept column scores at least `match`): no record
                    } else if (is_written(b, a) && _annotate) {
                        annotated(r, a, h.bucket_name[bucket_id], h.bucket_offsets[bucket_id] + static_cast<size_t>(offset < 0 ? 0 : offset), is_original,
                                  pair_flags, map_qual, {}, rnext, pnext, tlen);
                    } else if (is_written(b, a)) {
                        const int clipped = offset < 0 ? 0 : offset;
                        const size_t ref_offset = static_cast<size_t>(b.begin[a]) + h.bucket_offsets[bucket_id] + clipped;   // :576
                        cg.clear();
                        for (uint64_t x = b.cigar_offset[a]; x < b.cigar_offset[a + 1]; x++) {
                            cg += std::to_string(b.cigar[x] >> 4);
                            cg += "MID"[b.cigar[x] & 15u];
                        }
                        if (cg.empty()) cg = "*";
                        sam.record(b.reads[r].id, is_original ? 0 : 16, h.bucket_name[bucket_id], ref_offset + 1,
                                   static_cast<uint8_t>(map_qual), cg, b.reads[r].seq, b.reads[r].qual,
                                   best ? std::string_view(best_tag) : std::string_view());
                        mapped_locations++;
                    }
                    a++;
                }
                if (split) {
                    // --split: the chosen segments of which the final clip kept something, in chosen order; the first written
                    // one is the primary
                    const uint32_t a0 = b.group_offset[r], ms = _split_params.max_segments;
                    struct segment { uint32_t a; unsigned int mapq, bucket; size_t ref_base; bool is_original; };
                    std::vector<segment> segs;
                    for (uint32_t k = 0; k < b.split.n_seg[r]; k++) {
                        const uint32_t c = b.split.seg[r * ms + k];
                        if (nothing_kept(b, c)) continue;
                        const locate_t &loc = locate_res[b.first_read + r][c - a0];
                        const int offset = std::get<1>(loc);
                        segs.push_back({c, split_mapq(b.split.score[c], b.split.s2[r * ms + k]), std::get<0>(loc),
                                        h.bucket_offsets[std::get<0>(loc)] + static_cast<size_t>(offset < 0 ? 0 : offset), std::get<4>(loc)});
                    }
                    std::vector<std::string> sa(segs.size());
                    for (size_t i = 0; segs.size() > 1 && i < segs.size(); i++) {
                        const uint32_t s = b.ann_slot[segs[i].a];
                        append_sa_entry(sa[i], h.bucket_name[segs[i].bucket], b.ann.pos[s] + segs[i].ref_base, !segs[i].is_original,
                                        b.ann.xcigar.data() + b.ann.xcigar_offset[s], b.ann.xcigar_offset[s + 1] - b.ann.xcigar_offset[s],
                                        segs[i].mapq, b.ann.nm[s]);
                    }
                    std::string sa_tag;
                    for (size_t i = 0; i < segs.size(); i++) {
                        sa_tag.clear();
                        if (segs.size() > 1) {
                            sa_tag = "SA:Z:";
                            for (size_t o = 0; o < segs.size(); o++)
                                if (o != i) sa_tag += sa[o];
                        }
                        annotated(r, segs[i].a, h.bucket_name[segs[i].bucket], segs[i].ref_base, segs[i].is_original, i ? 0x800u : 0u,
                                  segs[i].mapq, sa_tag, "*", 0, 0);
                    }
                }
                if (rescued) {
                    const uint32_t ra = b.rescued_at[r];
                    if (is_written(b, ra) && !(_clip && nothing_kept(b, ra))) {
                        const auto [bucket, offset] = rescued_place(b, r);
                        annotated(r, ra, h.bucket_name[bucket], h.bucket_offsets[bucket] + static_cast<size_t>(offset), b.text_rc[ra] == 0, pair_flags,
                                  bq.mapq, "XR:i:1", rnext, pnext, tlen);
                    }
                }
            }
            b.reads.clear(); b.bases.clear();
            b.text_start.clear(); b.text_len.clear(); b.text_rc.clear(); b.query_start.clear(); b.query_len.clear();
            b.max_edits.clear();
            b.group_offset.assign(1, 0); b.margin.clear(); b.hint.clear(); b.contig.clear();
        };
        // the block just filled goes to the verifier as soon as the one before has left it; that one's records are written
        // while the verifier works
        auto flush = [&]() {
            if (in_flight >= 0) {
                worker.join();
                to_write = in_flight;
            }
            in_flight = cur;
            worker = std::thread(align, std::ref(blocks[cur]));
            cur ^= 1;
            if (to_write >= 0) {
                write(blocks[to_write]);
                to_write = -1;
            }
            blocks[cur].first_read = read_id;
        };
        try {
            for_each_fastq(sequence_file, [&](const FastqRecord &rec) {
                Block &b = blocks[cur];
                const size_t len = rec.seq.size();
                b.reads.push_back({std::string(rec.id), std::string(), std::string(rec.qual), b.bases.size()});
                if (paired) {
                    // QNAME without a trailing /1 or /2; the two mates share it (blocks are cut at even counts: the first mate
                    // is the read before in this block)
                    std::string &id = b.reads.back().id;
                    if (id.size() >= 2 && id[id.size() - 2] == '/' && (id.back() == '1' || id.back() == '2')) id.resize(id.size() - 2);
                    if (read_id % 2u && id != b.reads[b.reads.size() - 2].id)
                        throw std::runtime_error("records " + std::to_string(read_id - 1) + " and " + std::to_string(read_id) + " of " + sequence_file +
                                                 " are not mates: their names are '" + b.reads[b.reads.size() - 2].id + "' and '" + id + "'");
                }
                append_dna4(b.reads.back().seq, rec.seq);
                b.bases.insert(b.bases.end(), rec.seq.begin(), rec.seq.end());
                for (auto &[bucket_id, offset, segment_offset, votes, is_original] : locate_res[read_id]) {
                    (void)segment_offset; (void)votes;
                    const size_t clipped = offset < 0 ? 0 : static_cast<size_t>(offset);
                    const size_t bucket_size = blen_[bucket_id];
                    const size_t width = std::min(len + 1 + static_cast<size_t>(allowed_indel_rate * len),   // :550
                                                  bucket_size - std::min(clipped, bucket_size));
                    b.text_start.push_back(bstart_[bucket_id] + std::min(clipped, bucket_size));
                    b.text_len.push_back(static_cast<uint32_t>(width));
                    b.text_rc.push_back(is_original ? 0 : 1);                                               // :563-567
                    b.query_start.push_back(b.reads.back().start);
                    b.query_len.push_back(static_cast<uint32_t>(len));
                    if (paired || split) b.contig.push_back(bucket_ref[bucket_id]);
                    if (bounded) b.max_edits.push_back(static_cast<uint32_t>(std::min(_max_edit_rate * static_cast<float>(len), 4e9f)));
                }
                if (split) b.group_offset.push_back(static_cast<uint32_t>(b.text_start.size()));
                if (best) {
                    // the read's group: the hint is the candidate with the most locator votes, the first of them
                    uint32_t at = 0, most = 0, k = 0;
                    for (auto &[bucket_id, offset, segment_offset, votes, is_original] : locate_res[read_id]) {
                        (void)bucket_id; (void)offset; (void)segment_offset; (void)is_original;
                        if (k == 0 || votes > most) {
                            most = votes;
                            at = k;
                        }
                        k++;
                    }
                    b.group_offset.push_back(static_cast<uint32_t>(b.text_start.size()));
                    b.margin.push_back(std::max(1u, static_cast<uint32_t>(std::min(_best_margin * static_cast<float>(len), 4e9f))));
                    b.hint.push_back(at);
                }
                read_id++;
                if ((b.reads.size() >= block_reads || b.bases.size() >= block_bases) && !(paired && b.reads.size() % 2u)) flush();
            });
            flush();                                            // the last, possibly empty, block
            worker.join();
            in_flight = -1;
            write(blocks[cur ^ 1]);
        } catch (...) {
            if (worker.joinable()) worker.join();
            throw;
        }
        if (_clip_overlap)
            std::cerr << "[INFO]\t\tOverlap: " << _overlap_cut << " of " << _overlap_pairs << " pairs cut, " << _overlap_bases
                      << " bases clipped\n";
        return mapped_locations;
    }
};

}  // namespace bm
