// bmv_rescue.hip -- the kernels of bmv_rescue (bmv_rescue.hip.h), in a translation unit of its own like bmv_pair.hip.
#include "bmv_rescue.hip.h"

namespace bmv {

// The window of bmv.h: where the mate of job j may lie beside its anchor, cut to the anchor's contig.
__global__ __launch_bounds__(256) void bmv_rescue_plan_kernel(RescueJob J) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= J.n) return;
    int64_t la, ra;
    rescue_anchor(J, j, la, ra);
    const int64_t m = (int64_t)J.query_len[j], me = (int64_t)J.max_edits[j], k = me < m ? me : m;
    const int64_t c0 = (int64_t)J.contig_start[j], c1 = (int64_t)J.contig_end[j];
    int64_t ws, we;
    const bool anchor_rc = J.anchor_text_rc[j] != 0;
    if (!anchor_rc) {
        // the mate on the reverse strand: its left end x in [x_lo, x_hi]
        const int64_t x_lo = rescue_max(la, rescue_max(ra - m, la + J.min_frag - m)), x_hi = la + J.max_frag - m;
        ws = rescue_max(c0, x_lo);
        we = rescue_min(c1, x_hi + m + k);
    } else {
        // the mate on the forward strand: its right end z in [z_lo, z_hi]
        const int64_t z_lo = ra + m - J.max_frag, z_hi = rescue_min(la + m, rescue_min(ra, ra + m - J.min_frag));
        ws = rescue_max(c0, z_lo - m - k);
        we = rescue_min(c1, z_hi);
    }
    J.text_start[j] = (uint64_t)ws;
    J.text_len[j] = we > ws ? (uint32_t)(we - ws) : 0u;
    J.text_rc[j] = anchor_rc ? 0 : 1;
}

// The rule: d <= k, and bmv_pair's proper between the anchor and the rescued mate's view and end.
__global__ __launch_bounds__(256) void bmv_rescue_finish_kernel(RescueJob J) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= J.n) return;
    const uint32_t m = J.query_len[j], me = J.max_edits[j], k = me < m ? me : m, n = J.text_len[j];
    const uint32_t d = J.d[j];
    const bool within = n != 0u && m != 0u && d != kBestBeyond && d <= k;
    const uint32_t end = within ? J.end[j] : 0u;
    bool proper = false;
    if (within) {
        int64_t la, ra;
        rescue_anchor(J, j, la, ra);
        const int64_t ts = (int64_t)J.text_start[j];
        int64_t fl, fr, rl, rr;
        if (J.anchor_text_rc[j] == 0) {                         // the anchor forward, the mate reverse
            fl = la;
            fr = ra;
            rl = ts + (int64_t)n - (int64_t)end;
            rr = rl + (int64_t)m;
        } else {
            rl = la;
            rr = ra;
            fr = ts + (int64_t)end;
            fl = fr - (int64_t)m;
        }
        const int64_t frag = rr - fl;
        proper = fl <= rl && fr <= rr && frag >= J.min_frag && frag <= J.max_frag;
    }
    J.out_edits[j] = within ? d : kBestBeyond;
    J.out_end[j] = end;
    J.out_proper[j] = proper ? 1 : 0;
}

template __global__ void bmv_rescue_lane_kernel<1>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<2>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<3>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<4>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<5>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<6>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<7>(RescueJob);
template __global__ void bmv_rescue_lane_kernel<8>(RescueJob);

}  // namespace bmv
