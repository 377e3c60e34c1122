// gpu_alignment_verifier.h -- the MI355X alignment verifier (include/bmv.h) behind bm::alignment_verifier.
// Replaces seqan3::align_pairwise in the BM_ALIGN branch of bucket_locator::locate
// (bucket_map/locator/bucket_locator.h:520-528,569-576) for a whole block of candidates per call.
// Several devices: the genome is replicated and the block's alignments -- independent of each other, the
// reference runs them one by one (:560-589) -- are cut into contiguous ranges of equal cell count, one per
// device; each device is handed only the span of the read buffer its queries cover.
// A share that holds a candidate beyond the contexts' limits (reads of more than 65 536 bases, windows of more than
// 81 920) goes through bmv_align_long; every other share through bmv_align, exactly as before.
// Fails loudly (throws) when the device path fails: no CPU fallback.
#pragma once

#include "../../include/bmv.h"
#include "bucket_locator.h"
#include "device_pool.h"

#include <sstream>
#include <string>

namespace bm {

class gpu_alignment_verifier : public alignment_verifier {
    static constexpr uint32_t kMaxQuery = 65536, kMaxText = 81920;   // the ABI's limits: reads are not known yet
    std::vector<bmv_ctx *> ctx_;

    static void check(int rc, const char *what) {
        if (rc != BMV_OK) throw std::runtime_error(std::string(what) + bmv_last_error());
    }

public:
    explicit gpu_alignment_verifier(std::vector<int> devices = {0}) {
        bmv_params p{};
        p.max_query_len = kMaxQuery;
        p.max_text_len = kMaxText;
        for (int dev : devices) {
            p.device = dev;
            bmv_ctx *c = nullptr;
            if (bmv_create(&p, &c) != BMV_OK) {
                const std::string why = bmv_last_error();
                for (bmv_ctx *o : ctx_) bmv_destroy(o);
                throw std::runtime_error("cannot create the GPU alignment verifier on device " + std::to_string(dev) + ": " + why);
            }
            ctx_.push_back(c);
        }
    }
    ~gpu_alignment_verifier() override {
        for (bmv_ctx *c : ctx_) bmv_destroy(c);
    }

    void load_genome_records(const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records) override {
        for_each_device(ctx_.size(), [&](size_t d) { check(bmv_load_genome_records(ctx_[d], rec, rec_len, n_records), "uploading the genome failed: "); });
    }
    void load_genome(const uint8_t *bases, uint64_t n_bases) override {
        for_each_device(ctx_.size(), [&](size_t d) { check(bmv_load_genome(ctx_[d], bases, n_bases), "uploading the genome failed: "); });
    }

    void align(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
               const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
               std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
               std::vector<uint32_t> &cigar) override {
        run(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, nullptr, n, score, begin, cigar_offset, cigar);
    }
    // bmv_align_bounded per device: the same cut, the same stitching
    void align_bounded(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                       const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *max_edits,
                       uint32_t n, std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                       std::vector<uint32_t> &cigar) override {
        run(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, max_edits, n, score, begin, cigar_offset, cigar);
    }

    // bmv_align_best per device: the batch is cut at GROUP borders into ranges of roughly equal cell count, the per-alignment
    // results are stitched as run() stitches them, the winners rebased to batch indices
    void best(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
              const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n, const uint32_t *group_offset,
              uint32_t n_groups, const uint32_t *margin, const uint32_t *hint, std::vector<int32_t> &score,
              std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar,
              std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end) override {
        grouped(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, group_offset, n_groups, margin, hint, nullptr,
                score, begin, cigar_offset, cigar, winner, edits, end);
    }

    // bmv_align_paired per device: the same, the batch cut at PAIR borders (the groups 2p and 2p + 1 stay on one device); the
    // picks rebased like the winners
    void paired(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n, const uint32_t *group_offset,
                uint32_t n_groups, const uint32_t *margin, const uint32_t *hint, const uint32_t *contig, uint32_t min_frag,
                uint32_t max_frag, std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
                std::vector<uint32_t> &cigar, std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end,
                std::vector<uint32_t> &pick, std::vector<uint8_t> &proper, std::vector<uint64_t> &s1, std::vector<uint64_t> &s2) override {
        if (n_groups & 1u) throw std::runtime_error("paired: an odd number of groups");
        pair_io io{contig, min_frag, max_frag, &pick, &proper, &s1, &s2, 0, 0, nullptr};
        grouped(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, group_offset, n_groups, margin, hint, &io, score,
                begin, cigar_offset, cigar, winner, edits, end);
    }

    // bmv_paired_begin per device, the devices' span histograms added and one range derived from the sum, bmv_paired_finish
    // per device under that range: the range is the whole batch's, however the batch was cut
    void paired_auto(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                     const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n, const uint32_t *group_offset,
                     uint32_t n_groups, const uint32_t *margin, const uint32_t *hint, const uint32_t *contig, uint32_t cap,
                     uint32_t min_pairs, uint32_t fallback_min, uint32_t fallback_max, std::vector<int32_t> &score,
                     std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar,
                     std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end, std::vector<uint32_t> &pick,
                     std::vector<uint8_t> &proper, std::vector<uint64_t> &s1, std::vector<uint64_t> &s2, frag_learned &learned) override {
        if (n_groups & 1u) throw std::runtime_error("paired: an odd number of groups");
        if (cap < 1u || cap > 65535u) throw std::runtime_error("paired: a fragment cap is 1 .. 65535");
        pair_io io{contig, fallback_min, fallback_max, &pick, &proper, &s1, &s2, cap, min_pairs, &learned};
        grouped(reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, group_offset, n_groups, margin, hint, &io, score,
                begin, cigar_offset, cigar, winner, edits, end);
    }

    bool can_annotate() const override { return true; }

private:
    // what paired() takes and returns beyond best()
    struct pair_io {
        const uint32_t *contig;
        uint32_t min_frag, max_frag;
        std::vector<uint32_t> *pick;
        std::vector<uint8_t> *proper;
        std::vector<uint64_t> *s1, *s2;
        uint32_t cap, min_pairs;        // paired_auto(): learned != nullptr, and min_frag / max_frag are the fallback
        frag_learned *learned;
    };

    // best() (pairs == nullptr) and paired(): the unit the batch is cut at is a group, or a pair of groups
    void grouped(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n, const uint32_t *group_offset,
                 uint32_t n_groups, const uint32_t *margin, const uint32_t *hint, const pair_io *pairs, std::vector<int32_t> &score,
                 std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset, std::vector<uint32_t> &cigar,
                 std::vector<uint32_t> &winner, std::vector<uint32_t> &edits, std::vector<uint32_t> &end) {
        const size_t D = ctx_.size();
        const uint32_t unit = pairs ? 2u : 1u;
        const auto t0 = std::chrono::steady_clock::now();
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        score.assign(n, 0);
        begin.assign(n, 0);
        cigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        winner.assign(n_groups, kBeyond);
        edits.assign(n, kBeyond);
        end.assign(n, 0);
        if (pairs) {
            pairs->pick->assign(n_groups, kBeyond);
            pairs->proper->assign(n_groups / 2u, 0);
            pairs->s1->assign(n_groups / 2u, kPairNone);
            pairs->s2->assign(n_groups / 2u, kPairNone);
        }
        std::vector<uint32_t> cut = cut_by_cost(n_groups / unit, D, [&](uint32_t u) {
            uint64_t cells = 1;
            for (uint32_t a = group_offset[u * unit]; a < group_offset[(u + 1u) * unit]; a++) cells += static_cast<uint64_t>(query_len[a]) * text_len[a];
            return cells;
        });
        for (uint32_t &x : cut) x *= unit;                      // in groups
        std::vector<float> ms_pair(D, 0.f);
        std::vector<uint64_t> combinations(D, 0);
        std::vector<uint64_t> total(D, 0), cells(D, 0), dist_cells(D, 0);
        std::vector<float> ms(D, 0.f);
        std::vector<std::array<uint32_t, 5>> counts(D, std::array<uint32_t, 5>{});
        std::vector<std::vector<uint32_t>> offs(D);             // per range its groups, counted from its first alignment
        std::vector<share> shares(D);
        for (size_t d = 0; d < D; d++) {
            const uint32_t g0 = cut[d], ng = cut[d + 1] - cut[d];
            if (ng == 0) continue;
            const uint32_t a0 = group_offset[g0];
            shares[d] = slice(all, a0, group_offset[g0 + ng] - a0);
            if (D > 1) {
                offs[d].assign(group_offset + g0, group_offset + g0 + ng + 1);
                for (uint32_t &o : offs[d]) o -= a0;
            }
        }
        const bool learn_range = pairs && pairs->learned;
        uint32_t min_frag = pairs ? pairs->min_frag : 0u, max_frag = pairs ? pairs->max_frag : 0u;
        std::vector<float> ms_frag(D, 0.f);
        if (learn_range) {
            // the first half on every device, the histograms added, one range
            const size_t bins = static_cast<size_t>(pairs->cap) + 1u;
            std::vector<std::vector<uint64_t>> hist(D);
            for_each_device(D, [&](size_t d) {
                const uint32_t g0 = cut[d], ng = cut[d + 1] - cut[d];
                if (ng == 0) return;
                const share &s = shares[d];
                check(bmv_paired_begin(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, s.n,
                                       D > 1 ? offs[d].data() : group_offset, ng, margin + g0, hint ? hint + g0 : nullptr,
                                       pairs->contig ? pairs->contig + s.a0 : nullptr, pairs->cap),
                      "the GPU alignment verifier failed: ");
                hist[d].assign(bins, 0);
                check(bmv_frag(ctx_[d], nullptr, hist[d].data()), "reading the fragment spans failed: ");
                bmv_last_frag_stats(ctx_[d], &ms_frag[d], nullptr);
            });
            std::vector<uint64_t> whole(bins, 0);
            for (size_t d = 0; d < D; d++)
                for (size_t b = 0; b < hist[d].size(); b++) whole[b] += hist[d][b];
            *pairs->learned = learn(whole, pairs->min_pairs, pairs->min_frag, pairs->max_frag);
            min_frag = pairs->learned->applied_min;
            max_frag = pairs->learned->applied_max;
        }
        for_each_device(D, [&](size_t d) {
            const uint32_t g0 = cut[d], ng = cut[d + 1] - cut[d];
            if (ng == 0) return;
            const share &s = shares[d];
            const std::vector<uint32_t> &off = offs[d];
            if (learn_range) {
                check(bmv_paired_finish(ctx_[d], min_frag, max_frag, &total[d]), "the GPU alignment verifier failed: ");
                bmv_last_pair_stats(ctx_[d], &ms_pair[d], &combinations[d]);
            } else if (pairs) {
                check(bmv_align_paired(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, s.n,
                                       D > 1 ? off.data() : group_offset, ng, margin + g0, hint ? hint + g0 : nullptr,
                                       pairs->contig ? pairs->contig + s.a0 : nullptr, pairs->min_frag, pairs->max_frag, &total[d]),
                      "the GPU alignment verifier failed: ");
                bmv_last_pair_stats(ctx_[d], &ms_pair[d], &combinations[d]);
            } else
                check(bmv_align_best(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, s.n,
                                     D > 1 ? off.data() : group_offset, ng, margin + g0, hint ? hint + g0 : nullptr, &total[d]),
                      "the GPU alignment verifier failed: ");
            bmv_last_stats(ctx_[d], &ms[d], &cells[d]);
            bmv_last_best_stats(ctx_[d], &counts[d][0], &counts[d][1], &counts[d][2], &counts[d][3], &counts[d][4], &dist_cells[d], nullptr,
                                nullptr);
        });
        const std::vector<uint64_t> at = starts(total);
        cigar.assign(at[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t g0 = cut[d], ng = cut[d + 1] - cut[d];
            if (ng == 0) return;
            const uint32_t a0 = group_offset[g0], m = group_offset[g0 + ng] - a0;
            std::vector<uint64_t> off(static_cast<size_t>(m) + 1);
            check(bmv_results(ctx_[d], score.data() + a0, begin.data() + a0, off.data(), cigar.data() + at[d]),
                  "reading the verifier's results failed: ");
            check(bmv_best(ctx_[d], winner.data() + g0, edits.data() + a0, end.data() + a0), "reading the verifier's results failed: ");
            stitch(cigar_offset, a0, m, off, at[d]);
            for (uint32_t g = g0; g < g0 + ng; g++)
                if (winner[g] != kBeyond) winner[g] += a0;
            if (!pairs) return;
            check(bmv_pairs(ctx_[d], pairs->pick->data() + g0, pairs->proper->data() + g0 / 2u, pairs->s1->data() + g0 / 2u,
                            pairs->s2->data() + g0 / 2u, nullptr),
                  "reading the verifier's results failed: ");
            for (uint32_t g = g0; g < g0 + ng; g++)
                if ((*pairs->pick)[g] != kBeyond) (*pairs->pick)[g] += a0;
        });
        // (ranges are contiguous and in order: an empty range's alignments do not exist, so every offset is set but the last)
        cigar_offset[n] = at[D];
        std::array<uint64_t, 5> all_counts{};
        for (size_t d = 0; d < D; d++)
            for (size_t k = 0; k < 5; k++) all_counts[k] += counts[d][k];
        std::string pair_part;
        if (pairs) {
            float slowest = 0;
            for (const float x : ms_pair) slowest = std::max(slowest, x);
            pair_part = "the pair kernel " + std::to_string(sum(combinations)) + " combinations in " + std::to_string(slowest) + " ms; ";
            if (learn_range)
                pair_part += "the span and histogram kernels " + std::to_string(*std::max_element(ms_frag.begin(), ms_frag.end())) + " ms; ";
        }
        std::cerr << "[BENCHMARK]\tGPU alignment verification, " << (pairs ? "best per pair: " : "best per read: ") << n << " alignments in "
                  << n_groups << " groups, " << sum(cells) << " cells; " << all_counts[0] << " seeds, " << all_counts[1]
                  << " through the distance round (" << sum(dist_cells) << " cells, " << all_counts[2] << " beyond, " << all_counts[3]
                  << " undecided), " << all_counts[4] << " realigned; " << pair_part << timing(ms, t0);
    }

public:

    // bmv_annotate per device: the batch is cut exactly as run() cuts it and the packed arrays are stitched the same way
    void annotate(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                  const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                  const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, annotation &out) override {
        post_pass({reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n}, begin, cigar_offset, cigar, out, nullptr, 0, 0);
    }
    // bmv_clip per device: the same cut, the same stitching, with the score and the two clips per alignment
    void clip(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
              const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
              const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t penalty, clipping &out) override {
        post_pass({reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n}, begin, cigar_offset, cigar, out, &out, match,
                  penalty);
    }

    // bmv_overlap per device.  The alignments are first put in an order in which mates are neighbours and the cut between two
    // devices' shares never falls inside a pair, so a pair never straddles two shares; the rule looks at one pair at a time, so
    // the result does not depend on the number of devices.  The results come back in the caller's order.
    bool can_clip_overlap() const override { return true; }
    void clip_overlap(const uint8_t *genome, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                      const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                      const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *mate, const uint32_t *contig, uint32_t n,
                      uint32_t match, uint32_t penalty, clipping &out, std::vector<uint32_t> &cut, uint64_t &pairs_cut,
                      uint64_t &bases_cut) override {
        (void)genome;
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        const char *failed = "the GPU overlap pass failed: ";
        for (uint32_t a = 0; a < n; a++)
            if (mate[a] != BMV_NO_MATE && (mate[a] >= n || mate[a] == a || mate[mate[a]] != a))
                throw std::runtime_error(std::string(failed) + "alignment " + std::to_string(a) + " and its mate do not name each other");
        // the batch as the devices see it: the caller's (one device), or a copy with mates side by side
        std::vector<uint32_t> order, p_tl, p_ql, p_bg, p_cg, p_mate, p_contig;
        std::vector<uint64_t> p_ts, p_qs, p_co;
        std::vector<uint8_t> p_trc;
        if (D > 1) {
            std::vector<uint32_t> where(n);
            for (uint32_t a = 0; a < n; a++) {
                if (mate[a] != BMV_NO_MATE && mate[a] < a) continue;
                where[a] = static_cast<uint32_t>(order.size());
                order.push_back(a);
                if (mate[a] == BMV_NO_MATE) continue;
                where[mate[a]] = static_cast<uint32_t>(order.size());
                order.push_back(mate[a]);
            }
            p_co.push_back(0);
            for (const uint32_t a : order) {
                p_ts.push_back(text_start[a]); p_tl.push_back(text_len[a]); p_trc.push_back(text_rc[a]);
                p_qs.push_back(query_start[a]); p_ql.push_back(query_len[a]); p_bg.push_back(begin[a]);
                p_mate.push_back(mate[a] == BMV_NO_MATE ? BMV_NO_MATE : where[mate[a]]);
                if (contig) p_contig.push_back(contig[a]);
                p_cg.insert(p_cg.end(), cigar + cigar_offset[a], cigar + cigar_offset[a + 1]);
                p_co.push_back(p_cg.size());
            }
            text_start = p_ts.data(); text_len = p_tl.data(); text_rc = p_trc.data(); query_start = p_qs.data(); query_len = p_ql.data();
            begin = p_bg.data(); cigar_offset = p_co.data(); cigar = p_cg.data(); mate = p_mate.data();
            if (contig) contig = p_contig.data();
        }
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        std::vector<uint32_t> share_at =
            cut_by_cost(n, D, [&](uint32_t a) { return static_cast<uint64_t>(all.query_len[a]) * all.text_len[a] + 1u; });
        for (size_t d = 1; d < D; d++)
            if (share_at[d] > 0 && share_at[d] < n && mate[share_at[d] - 1u] == share_at[d]) share_at[d]++;
        clipping got;                                           // in the devices' order
        std::vector<uint32_t> got_cut(n, 0);
        got.score.assign(n, 0);
        got.clip_left.assign(n, 0);
        got.clip_right.assign(n, 0);
        got.nm.assign(n, 0);
        got.pos.assign(n, 0);
        got.ref_len.assign(n, 0);
        got.xcigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        got.ref_offset.assign(static_cast<size_t>(n) + 1, 0);
        std::vector<uint64_t> n_x(D, 0), n_r(D, 0), columns(D, 0), pairs(D, 0), bases(D, 0);
        std::vector<float> ms(D, 0.f);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = share_at[d], m = share_at[d + 1] - share_at[d];
            if (m == 0) return;
            const share s = slice(all, a0, m);
            std::vector<uint32_t> local(mate + a0, mate + a0 + m);      // the mates' places inside the share
            for (uint32_t &x : local)
                if (x != BMV_NO_MATE) x -= a0;
            check(bmv_overlap(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len,
                              begin + a0, cigar_offset + a0, cigar, local.data(), contig ? contig + a0 : nullptr, s.n, match, penalty,
                              &n_x[d], &n_r[d]), failed);
            bmv_last_overlap_stats(ctx_[d], &ms[d], &columns[d], &pairs[d], &bases[d]);
        });
        const std::vector<uint64_t> at_x = starts(n_x), at_r = starts(n_r);
        got.xcigar.assign(at_x[D], 0);
        got.ref_bases.assign(at_r[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = share_at[d], m = share_at[d + 1] - share_at[d];
            if (m == 0) return;
            std::vector<uint64_t> xo(static_cast<size_t>(m) + 1), ro(static_cast<size_t>(m) + 1);
            check(bmv_overlapped(ctx_[d], got.score.data() + a0, got.clip_left.data() + a0, got.clip_right.data() + a0, got.nm.data() + a0,
                                 got.pos.data() + a0, got.ref_len.data() + a0, xo.data(), got.xcigar.data() + at_x[d], ro.data(),
                                 got.ref_bases.data() + at_r[d], got_cut.data() + a0),
                  "reading the overlap-clipped alignments failed: ");
            stitch(got.xcigar_offset, a0, m, xo, at_x[d]);
            stitch(got.ref_offset, a0, m, ro, at_r[d]);
        });
        got.xcigar_offset[n] = at_x[D];
        got.ref_offset[n] = at_r[D];
        if (D == 1) {
            out = std::move(got);
            cut = std::move(got_cut);
        } else {                                                // back into the caller's order
            out.score.assign(n, 0); out.clip_left.assign(n, 0); out.clip_right.assign(n, 0);
            out.nm.assign(n, 0); out.pos.assign(n, 0); out.ref_len.assign(n, 0);
            cut.assign(n, 0);
            out.xcigar_offset.assign(static_cast<size_t>(n) + 1, 0);
            out.ref_offset.assign(static_cast<size_t>(n) + 1, 0);
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t a = order[k];
                out.score[a] = got.score[k]; out.clip_left[a] = got.clip_left[k]; out.clip_right[a] = got.clip_right[k];
                out.nm[a] = got.nm[k]; out.pos[a] = got.pos[k]; out.ref_len[a] = got.ref_len[k];
                cut[a] = got_cut[k];
                out.xcigar_offset[a + 1] = got.xcigar_offset[k + 1] - got.xcigar_offset[k];
                out.ref_offset[a + 1] = got.ref_offset[k + 1] - got.ref_offset[k];
            }
            for (uint32_t a = 0; a < n; a++) {
                out.xcigar_offset[a + 1] += out.xcigar_offset[a];
                out.ref_offset[a + 1] += out.ref_offset[a];
            }
            out.xcigar.assign(got.xcigar.size(), 0);
            out.ref_bases.assign(got.ref_bases.size(), 0);
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t a = order[k];
                std::copy(got.xcigar.begin() + static_cast<ptrdiff_t>(got.xcigar_offset[k]),
                          got.xcigar.begin() + static_cast<ptrdiff_t>(got.xcigar_offset[k + 1]),
                          out.xcigar.begin() + static_cast<ptrdiff_t>(out.xcigar_offset[a]));
                std::copy(got.ref_bases.begin() + static_cast<ptrdiff_t>(got.ref_offset[k]),
                          got.ref_bases.begin() + static_cast<ptrdiff_t>(got.ref_offset[k + 1]),
                          out.ref_bases.begin() + static_cast<ptrdiff_t>(out.ref_offset[a]));
            }
        }
        pairs_cut = sum(pairs);
        bases_cut = sum(bases);
        std::cerr << "[BENCHMARK]\tGPU overlap clipping: " << n << " alignments, " << sum(columns) << " columns, " << pairs_cut
                  << " pairs cut; " << timing(ms, t0);
    }

    // bmv_split per device: the batch is cut at GROUP borders into ranges of about equal column count (a read's candidates stay
    // on one device: the pick compares them with each other); the chosen indices are rebased to the batch
    void split(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc,
               const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin, const uint64_t *cigar_offset,
               const uint32_t *cigar, const uint32_t *contig, uint32_t n, const uint32_t *group_offset, uint32_t n_groups,
               const split_params &p, split_result &out) override {
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        const size_t ms = p.max_segments;
        out.score.assign(n, 0);
        out.q_lo.assign(n, 0);
        out.q_hi.assign(n, 0);
        out.g_lo.assign(n, 0);
        out.g_hi.assign(n, 0);
        out.n_seg.assign(n_groups, 0);
        out.seg.assign(n_groups * ms, kSplitBeyond);
        out.s2.assign(n_groups * ms, kSplitNone);
        const std::vector<uint32_t> cut = cut_by_cost(n_groups, D, [&](uint32_t g) {
            uint64_t columns = 1;
            for (uint64_t x = cigar_offset[group_offset[g]]; x < cigar_offset[group_offset[g + 1]]; x++) columns += cigar[x] >> 4;
            return columns;
        });
        std::vector<float> ms_range(D, 0.f), ms_pick(D, 0.f);
        std::vector<uint64_t> columns(D, 0), segments(D, 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t g0 = cut[d], ng = cut[d + 1] - cut[d];
            if (ng == 0) return;
            const uint32_t a0 = group_offset[g0];
            const share s = slice(all, a0, group_offset[g0 + ng] - a0);
            std::vector<uint32_t> off;                          // the range's groups, counted from its first alignment
            if (D > 1) {
                off.assign(group_offset + g0, group_offset + g0 + ng + 1);
                for (uint32_t &o : off) o -= a0;
            }
            check(bmv_split(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, begin + s.a0,
                            cigar_offset + s.a0, cigar, contig ? contig + s.a0 : nullptr, s.n, D > 1 ? off.data() : group_offset, ng, p.match,
                            p.penalty, p.min_score, p.max_overlap_permille, p.max_segments),
                  "the GPU split pass failed: ");
            check(bmv_segments(ctx_[d], out.score.data() + a0, out.q_lo.data() + a0, out.q_hi.data() + a0, out.g_lo.data() + a0,
                               out.g_hi.data() + a0, out.n_seg.data() + g0, out.seg.data() + g0 * ms, out.s2.data() + g0 * ms),
                  "reading the split alignments failed: ");
            for (size_t x = g0 * ms; x < (g0 + ng) * ms; x++)
                if (out.seg[x] != kSplitBeyond) out.seg[x] += a0;
            float r = 0.f, k = 0.f;
            bmv_last_split_stats(ctx_[d], &r, &k, &columns[d], &segments[d]);
            ms_range[d] = r;
            ms_pick[d] = k;
        });
        std::vector<float> both(D, 0.f);
        for (size_t d = 0; d < D; d++) both[d] = ms_range[d] + ms_pick[d];
        std::cerr << "[BENCHMARK]\tGPU split alignments: " << n << " alignments in " << n_groups << " groups, " << sum(columns) << " columns, "
                  << sum(segments) << " segments; range pass " << *std::max_element(ms_range.begin(), ms_range.end()) << " ms, pick "
                  << *std::max_element(ms_pick.begin(), ms_pick.end()) << " ms; " << timing(both, t0);
    }

    // bmv_realign per device: the same cut, the results stitched as run() stitches the aligners'
    bool can_realign() const override { return true; }
    void realign(const uint8_t *, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                 const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, const affine_scores &sc, realignment &out) override {
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        out.score.assign(n, 0);
        out.begin.assign(n, 0);
        out.realigned.assign(n, 0);
        out.cigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        const std::vector<uint32_t> cut = cut_by_cost(n, D, [&](uint32_t a) { return static_cast<uint64_t>(query_len[a]) + 1u; });
        std::vector<uint64_t> total(D, 0), cells(D, 0);
        std::vector<float> ms(D, 0.f);
        std::vector<uint32_t> passed(D, 0);
        for_each_device(D, [&](size_t d) {
            if (cut[d + 1] == cut[d]) return;
            const share s = slice(all, cut[d], cut[d + 1] - cut[d]);
            check(bmv_realign(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, begin + s.a0,
                              cigar_offset + s.a0, cigar, s.n, sc.match, sc.mismatch, sc.gap_open, sc.gap_extend, sc.band, &total[d]),
                  "the GPU realignment pass failed: ");
            bmv_last_realign_stats(ctx_[d], &ms[d], &cells[d], &passed[d]);
        });
        const std::vector<uint64_t> at = starts(total);
        out.cigar.assign(at[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            std::vector<uint64_t> off(static_cast<size_t>(m) + 1);
            check(bmv_realigned(ctx_[d], out.score.data() + a0, out.begin.data() + a0, out.realigned.data() + a0, off.data(),
                                out.cigar.data() + at[d]),
                  "reading the realigned alignments failed: ");
            stitch(out.cigar_offset, a0, m, off, at[d]);
        });
        out.cigar_offset[n] = at[D];
        std::cerr << "[BENCHMARK]\tGPU affine realignment: " << n << " alignments, " << sum(cells) << " band cells, " << sum(passed)
                  << " passed through; " << timing(ms, t0);
    }

    // bmv_leftalign per device: the same cut, the results stitched the same way
    bool can_left_align() const override { return true; }
    void left_align(const uint8_t *, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                    const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                    const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, left_alignment &out) override {
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        out.begin.assign(n, 0);
        out.dropped.assign(n, 0);
        out.changed.assign(n, 0);
        out.cigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        const std::vector<uint32_t> cut = cut_by_cost(n, D, [&](uint32_t a) { return cigar_offset[a + 1] - cigar_offset[a] + 1u; });
        std::vector<uint64_t> total(D, 0), compared(D, 0), merges(D, 0), dropped(D, 0);
        std::vector<float> ms(D, 0.f);
        std::vector<uint32_t> changed(D, 0);
        for_each_device(D, [&](size_t d) {
            if (cut[d + 1] == cut[d]) return;
            const share s = slice(all, cut[d], cut[d + 1] - cut[d]);
            check(bmv_leftalign(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len, begin + s.a0,
                                cigar_offset + s.a0, cigar, s.n, &total[d]),
                  "the GPU indel normalisation pass failed: ");
            bmv_last_leftalign_stats(ctx_[d], &ms[d], &compared[d], &changed[d], &merges[d], &dropped[d]);
        });
        const std::vector<uint64_t> at = starts(total);
        out.cigar.assign(at[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            std::vector<uint64_t> off(static_cast<size_t>(m) + 1);
            check(bmv_leftaligned(ctx_[d], out.begin.data() + a0, off.data(), out.cigar.data() + at[d], out.changed.data() + a0,
                                  out.dropped.data() + a0),
                  "reading the normalised alignments failed: ");
            stitch(out.cigar_offset, a0, m, off, at[d]);
        });
        out.cigar_offset[n] = at[D];
        out.compared = sum(compared);
        out.merges = sum(merges);
        std::cerr << "[BENCHMARK]\tGPU indel normalisation: " << n << " alignments, " << sum(changed) << " changed, " << out.compared
                  << " columns compared, " << out.merges << " merges, " << sum(dropped) << " bases dropped; " << timing(ms, t0);
    }

    // bmv_rescue per device: the jobs -- independent of each other -- in contiguous ranges of equal cost, each device handed
    // the span of the read buffer its queries cover
    void rescue(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *anchor_text_start, const uint32_t *anchor_text_len,
                const uint8_t *anchor_text_rc, const uint32_t *anchor_query_len, const uint32_t *anchor_end, const uint64_t *contig_start,
                const uint64_t *contig_end, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *max_edits, uint32_t n,
                uint32_t min_frag, uint32_t max_frag, rescued &out) override {
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        out.text_start.assign(n, 0);
        out.text_len.assign(n, 0);
        out.text_rc.assign(n, 0);
        out.edits.assign(n, kBeyond);
        out.end.assign(n, 0);
        out.proper.assign(n, 0);
        const std::vector<uint32_t> cut = cut_by_cost(n, D, [&](uint32_t j) { return static_cast<uint64_t>(query_len[j]) + 1u; });
        std::vector<float> ms(D, 0.f);
        std::vector<uint64_t> cells(D, 0);
        std::vector<uint32_t> parts(D, 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t j0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            uint64_t lo = 0, hi = n_read_bytes;
            std::vector<uint64_t> rebased;
            if (D > 1) {
                lo = ~0ull, hi = 0;
                for (uint32_t j = j0; j < j0 + m; j++) {
                    lo = std::min(lo, query_start[j]);
                    hi = std::max(hi, query_start[j] + query_len[j]);
                }
                rebased.assign(query_start + j0, query_start + j0 + m);
                for (uint64_t &q : rebased) q -= lo;
            }
            check(bmv_rescue(ctx_[d], reads + lo, hi - lo, anchor_text_start + j0, anchor_text_len + j0, anchor_text_rc + j0,
                             anchor_query_len + j0, anchor_end + j0, contig_start + j0, contig_end + j0,
                             D > 1 ? rebased.data() : query_start, query_len + j0, max_edits + j0, m, min_frag, max_frag),
                  "the GPU mate rescue failed: ");
            check(bmv_rescued(ctx_[d], out.text_start.data() + j0, out.text_len.data() + j0, out.text_rc.data() + j0, out.edits.data() + j0,
                              out.end.data() + j0, out.proper.data() + j0),
                  "reading the rescued mates failed: ");
            bmv_last_rescue_stats(ctx_[d], &ms[d], &cells[d], &parts[d]);
        });
        uint32_t rescued_n = 0;
        for (uint32_t j = 0; j < n; j++) rescued_n += out.proper[j] ? 1u : 0u;
        std::cerr << "[BENCHMARK]\tGPU mate rescue: " << n << " jobs, " << sum(cells) << " cells, " << *std::max_element(parts.begin(), parts.end())
                  << " parts a job; " << rescued_n << " within bound and proper; " << timing(ms, t0);
    }

private:
    // the views of a batch, as every call of the ABI takes them
    struct batch {
        const uint8_t *reads;
        uint64_t n_read_bytes;
        const uint64_t *text_start;
        const uint32_t *text_len;
        const uint8_t *text_rc;
        const uint64_t *query_start;
        const uint32_t *query_len;
        uint32_t n;
    };
    // What one device is handed of a batch: the alignments a0 .. a0 + n.  Arrays the share does not hold (edit bounds, begins,
    // CIGAR offsets) go with it as `array + a0`.
    struct share : batch {
        uint32_t a0 = 0;
        std::vector<uint64_t> rebased;      // several devices: what query_start points to, counted from the share's first read byte
        share() = default;
        share(share &&) = default;          // (a move keeps the vector's storage; a copy would leave query_start behind)
        share &operator=(share &&) = default;
    };
    // One device: the whole batch as it came, no copies (a0 = 0, n = the batch's).  Several: only the span lo .. hi of the read
    // buffer the share's queries cover, query_start rebased to it, every pointer advanced by a0.
    share slice(const batch &b, uint32_t a0, uint32_t m) const {
        share s;
        static_cast<batch &>(s) = b;
        if (ctx_.size() == 1) return s;
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t a = a0; a < a0 + m; a++) {
            lo = std::min(lo, b.query_start[a]);
            hi = std::max(hi, b.query_start[a] + b.query_len[a]);
        }
        if (m == 0) lo = 0;
        s.rebased.assign(b.query_start + a0, b.query_start + a0 + m);
        for (uint64_t &q : s.rebased) q -= lo;
        s.reads = b.reads + lo;
        s.n_read_bytes = hi - lo;
        s.text_start = b.text_start + a0;
        s.text_len = b.text_len + a0;
        s.text_rc = b.text_rc + a0;
        s.query_start = s.rebased.data();
        s.query_len = b.query_len + a0;
        s.n = m;
        s.a0 = a0;
        return s;
    }
    // Packed arrays of the ranges back to back, in range order: where each range's entries begin (and, last, how many there are) ...
    static std::vector<uint64_t> starts(const std::vector<uint64_t> &total) {
        std::vector<uint64_t> at(total.size() + 1, 0);
        for (size_t d = 0; d < total.size(); d++) at[d + 1] = at[d] + total[d];
        return at;
    }
    // ... and the offsets of a range's m alignments from a0 on, which count from its own first entry, rebased by `at`
    static void stitch(std::vector<uint64_t> &offset, uint32_t a0, uint32_t m, const std::vector<uint64_t> &of_range, uint64_t at) {
        for (uint32_t a = 0; a < m; a++) offset[a0 + a] = at + of_range[a];
    }
    template <typename T>
    static uint64_t sum(const std::vector<T> &per_device) {
        uint64_t all = 0;
        for (const T &x : per_device) all += x;
        return all;
    }
    // the end of every [BENCHMARK] line: the kernels' time on the slowest device, of the call's
    static std::string timing(const std::vector<float> &ms, std::chrono::steady_clock::time_point t0) {
        const size_t D = ms.size();
        float slowest = 0;
        for (const float x : ms) slowest = std::max(slowest, x);
        const float call_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::ostringstream out;
        out << "kernels " << slowest << " ms" << (D > 1 ? " on the slowest of " + std::to_string(D) + " devices," : "") << " of "
            << call_ms << " ms in the call.\n";
        return out.str();
    }

    // clipped == nullptr: bmv_annotate; else bmv_clip under (match, penalty), `clipped` being `out` itself
    void post_pass(const batch &all, const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar, annotation &out,
                   clipping *clipped, uint32_t match, uint32_t penalty) {
        const size_t D = ctx_.size();
        const uint32_t n = all.n;
        const auto t0 = std::chrono::steady_clock::now();
        const char *failed = clipped ? "the GPU clipping pass failed: " : "the GPU annotation pass failed: ";
        out.nm.assign(n, 0);
        out.pos.assign(n, 0);
        out.ref_len.assign(n, 0);
        out.xcigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        out.ref_offset.assign(static_cast<size_t>(n) + 1, 0);
        if (clipped) {
            clipped->score.assign(n, 0);
            clipped->clip_left.assign(n, 0);
            clipped->clip_right.assign(n, 0);
        }
        const std::vector<uint32_t> cut =
            cut_by_cost(n, D, [&](uint32_t a) { return static_cast<uint64_t>(all.query_len[a]) * all.text_len[a] + 1u; });
        std::vector<uint64_t> n_x(D, 0), n_r(D, 0), columns(D, 0);
        std::vector<float> ms(D, 0.f);
        for_each_device(D, [&](size_t d) {
            if (cut[d + 1] == cut[d]) return;
            const share s = slice(all, cut[d], cut[d + 1] - cut[d]);
            if (clipped) {
                check(bmv_clip(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len,
                               begin + s.a0, cigar_offset + s.a0, cigar, s.n, match, penalty, &n_x[d], &n_r[d]), failed);
                bmv_last_clip_stats(ctx_[d], &ms[d], &columns[d]);
            } else {
                check(bmv_annotate(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len,
                                   begin + s.a0, cigar_offset + s.a0, cigar, s.n, &n_x[d], &n_r[d]), failed);
                bmv_last_annotate_stats(ctx_[d], &ms[d], &columns[d]);
            }
        });
        const std::vector<uint64_t> at_x = starts(n_x), at_r = starts(n_r);
        out.xcigar.assign(at_x[D], 0);
        out.ref_bases.assign(at_r[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            std::vector<uint64_t> xo(static_cast<size_t>(m) + 1), ro(static_cast<size_t>(m) + 1);
            if (clipped)
                check(bmv_clipped(ctx_[d], clipped->score.data() + a0, clipped->clip_left.data() + a0, clipped->clip_right.data() + a0,
                                  out.nm.data() + a0, out.pos.data() + a0, out.ref_len.data() + a0, xo.data(),
                                  out.xcigar.data() + at_x[d], ro.data(), out.ref_bases.data() + at_r[d]),
                      "reading the clipped alignments failed: ");
            else
                check(bmv_annotations(ctx_[d], out.nm.data() + a0, out.pos.data() + a0, out.ref_len.data() + a0, xo.data(),
                                      out.xcigar.data() + at_x[d], ro.data(), out.ref_bases.data() + at_r[d]),
                      "reading the annotations failed: ");
            stitch(out.xcigar_offset, a0, m, xo, at_x[d]);
            stitch(out.ref_offset, a0, m, ro, at_r[d]);
        });
        out.xcigar_offset[n] = at_x[D];
        out.ref_offset[n] = at_r[D];
        std::cerr << "[BENCHMARK]\tGPU alignment " << (clipped ? "clipping: " : "annotation: ") << n << " alignments, " << sum(columns)
                  << " columns; " << timing(ms, t0);
    }

    // max_edits == nullptr: bmv_align / bmv_align_long, exactly as before
    void run(const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
             const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *max_edits, uint32_t n,
             std::vector<int32_t> &score, std::vector<uint32_t> &begin, std::vector<uint64_t> &cigar_offset,
             std::vector<uint32_t> &cigar) {
        const size_t D = ctx_.size();
        const auto t0 = std::chrono::steady_clock::now();
        const batch all{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
        score.assign(n, 0);
        begin.assign(n, 0);
        cigar_offset.assign(static_cast<size_t>(n) + 1, 0);
        const std::vector<uint32_t> cut =
            cut_by_cost(n, D, [&](uint32_t a) { return static_cast<uint64_t>(query_len[a]) * text_len[a] + 1u; });
        std::vector<uint64_t> total(D, 0), cells(D, 0);
        std::vector<float> ms(D, 0.f);
        std::vector<uint32_t> rejected(D, 0);
        std::vector<uint64_t> screened(D, 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            bool beyond = false;                                // a candidate bmv_align cannot take: the share goes long
            for (uint32_t a = a0; a < a0 + m; a++) beyond = beyond || query_len[a] > kMaxQuery || text_len[a] > kMaxText;
            const share s = slice(all, a0, m);
            if (max_edits)
                check(bmv_align_bounded(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc, s.query_start, s.query_len,
                                        max_edits + s.a0, s.n, &total[d]), "the GPU alignment verifier failed: ");
            else
                check((beyond ? bmv_align_long : bmv_align)(ctx_[d], s.reads, s.n_read_bytes, s.text_start, s.text_len, s.text_rc,
                                                            s.query_start, s.query_len, s.n, &total[d]),
                      "the GPU alignment verifier failed: ");
            bmv_last_stats(ctx_[d], &ms[d], &cells[d]);
            if (max_edits) bmv_last_bounded_stats(ctx_[d], &rejected[d], &screened[d], nullptr);
        });
        // CIGARs of the ranges back to back, in range order; a range's offsets count from its own first entry
        const std::vector<uint64_t> at = starts(total);
        cigar.assign(at[D], 0);
        for_each_device(D, [&](size_t d) {
            const uint32_t a0 = cut[d], m = cut[d + 1] - cut[d];
            if (m == 0) return;
            std::vector<uint64_t> off(static_cast<size_t>(m) + 1);
            check(bmv_results(ctx_[d], score.data() + a0, begin.data() + a0, off.data(), cigar.data() + at[d]),
                  "reading the verifier's results failed: ");
            stitch(cigar_offset, a0, m, off, at[d]);
        });
        cigar_offset[n] = at[D];
        std::cerr << "[BENCHMARK]\tGPU alignment verification: " << n << " alignments, " << sum(cells) << " cells"
                  << (max_edits ? ", " + std::to_string(sum(rejected)) + " rejected by the edit bound after " + std::to_string(sum(screened)) +
                                      " screen cells" : std::string())
                  << "; " << timing(ms, t0);
    }
};

}  // namespace bm
