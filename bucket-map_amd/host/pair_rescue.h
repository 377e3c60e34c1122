// pair_rescue.h -- `bucketmap_align --rescue`: mate rescue as bmv_rescue defines it (include/bmv.h), restated for the host
// (alignment_verifier::rescue's default plans with it), and the rule by which the locator gives a pair its jobs and keeps a
// result.  The Python restatements are bucket_map_amd.verify.rescue_window and bucket_map_amd.verify.select_rescue.
//
// The window.  The anchor is a known alignment of the partner, given as bmv_pair takes one; La, Ra are its L and R by
// pair_mapq.h's two formulas; m is the mate's length, k = min(max_edits, m), [c0, c1) the anchor's contig, everything signed
// 64-bit in the concatenated genome.
//   anchor forward    the mate is sought on the reverse strand; its left end x lies in [x_lo, x_hi] with
//                     x_lo = max(La, Ra - m, La + min_frag - m) and x_hi = La + max_frag - m; the view is
//                     [max(c0, x_lo), min(c1, x_hi + m + k))
//   anchor reverse    the mate is sought forward; its right end z lies in [z_lo, z_hi] with z_lo = Ra + m - max_frag and
//                     z_hi = min(La + m, Ra, Ra + m - min_frag); the view is [max(c0, z_lo - m - k), min(c1, z_hi))
// The jobs.  A pair that bmv_pair did not find proper gets job i -- anchored on mate i's own winner, its query the OTHER mate,
// max_edits = rescue_bound(rate, the other's length) -- when that winner is known with edits <= rescue_bound(rate, its
// length).  A job counts when it comes back within bound and proper; of two that count the smaller anchor edits + rescued
// edits wins, and a tie goes to job 0.  The scale of `rate` is a choice, as the MAPQ scales are.
#pragma once

#include "pair_mapq.h"

#include <algorithm>
#include <cstdint>

namespace bm {

struct rescue_view {
    uint64_t text_start;
    uint32_t text_len;
    uint8_t text_rc;
};

inline rescue_view rescue_window(uint64_t anchor_text_start, uint32_t anchor_text_len, bool anchor_text_rc, uint32_t anchor_query_len,
                                 uint32_t anchor_end, uint64_t contig_start, uint64_t contig_end, uint32_t query_len, uint32_t max_edits,
                                 uint32_t min_frag, uint32_t max_frag) {
    const int64_t ts = static_cast<int64_t>(anchor_text_start), m = query_len, k = std::min(max_edits, query_len);
    const int64_t c0 = static_cast<int64_t>(contig_start), c1 = static_cast<int64_t>(contig_end), lo = min_frag, hi = max_frag;
    int64_t la, ra, ws, we;
    if (anchor_text_rc) {
        la = ts + anchor_text_len - anchor_end;
        ra = la + anchor_query_len;
        const int64_t z_lo = ra + m - hi, z_hi = std::min({la + m, ra, ra + m - lo});
        ws = std::max(c0, z_lo - m - k);
        we = std::min(c1, z_hi);
    } else {
        ra = ts + anchor_end;
        la = ra - anchor_query_len;
        const int64_t x_lo = std::max({la, ra - m, la + lo - m}), x_hi = la + hi - m;
        ws = std::max(c0, x_lo);
        we = std::min(c1, x_hi + m + k);
    }
    return {static_cast<uint64_t>(ws), we > ws ? static_cast<uint32_t>(we - ws) : 0u, static_cast<uint8_t>(anchor_text_rc ? 0 : 1)};
}

// bmv_pair's proper between the anchor and the rescued mate, the latter given by its view and end column
inline bool rescue_proper(uint64_t anchor_text_start, uint32_t anchor_text_len, bool anchor_text_rc, uint32_t anchor_query_len,
                          uint32_t anchor_end, const rescue_view &v, uint32_t query_len, uint32_t end, uint32_t min_frag, uint32_t max_frag) {
    const int64_t ts = static_cast<int64_t>(anchor_text_start), vs = static_cast<int64_t>(v.text_start);
    int64_t fl, fr, rl, rr;
    if (anchor_text_rc) {
        rl = ts + anchor_text_len - anchor_end;
        rr = rl + anchor_query_len;
        fr = vs + end;
        fl = fr - query_len;
    } else {
        fr = ts + anchor_end;
        fl = fr - anchor_query_len;
        rl = vs + v.text_len - end;
        rr = rl + query_len;
    }
    const int64_t frag = rr - fl;
    return fl <= rl && fr <= rr && frag >= static_cast<int64_t>(min_frag) && frag <= static_cast<int64_t>(max_frag);
}

// (uint32_t)(rate x length), in single precision
inline uint32_t rescue_bound(float rate, uint32_t length) { return static_cast<uint32_t>(std::min(rate * static_cast<float>(length), 4e9f)); }

struct rescue_choice {
    bool job[2];            // job i: anchored on mate i, its query the other mate
    uint32_t max_edits[2];  // of job i
    int keep;               // -1, or the job whose result the pair keeps
};

// anchor_edits[i]: the edits of mate i's own winner, kBestBeyond when it has none.  rescued_edits / rescued_proper: the
// results of the two jobs (ignored where there is no job), or null before they are known.
inline rescue_choice select_rescue(bool proper, const uint32_t anchor_edits[2], const uint32_t read_len[2], float rate,
                                   const uint32_t *rescued_edits, const uint8_t *rescued_proper) {
    rescue_choice out{{false, false}, {rescue_bound(rate, read_len[1]), rescue_bound(rate, read_len[0])}, -1};
    if (proper) return out;
    for (int i = 0; i < 2; i++) out.job[i] = anchor_edits[i] != kBestBeyond && anchor_edits[i] <= rescue_bound(rate, read_len[i]);
    if (!rescued_edits) return out;
    uint64_t best = 0;
    for (int i = 0; i < 2; i++) {
        if (!out.job[i] || rescued_edits[i] == kBestBeyond || !rescued_proper[i]) continue;
        const uint64_t total = static_cast<uint64_t>(anchor_edits[i]) + rescued_edits[i];
        if (out.keep < 0 || total < best) {
            out.keep = i;
            best = total;
        }
    }
    return out;
}

}  // namespace bm
