// bmg_ctx.hip.h -- what a bmg_ctx is, for the translation units of libbmf.so that read the genotype caller's state on the
// device: bmg_api.hip, which owns it, and bmr_api.hip (include/bmr.h), which streams the cells of every position once.  It
// is internal like bms_ctx.hip.h: include/bmg.h exports no more than it did.
#pragma once

#include "bm_hip_util.h"
#include "bmg_rule.hip.h"

struct bmg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool begun = false;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    bmg::params pr{0, 13, 30, 60, 3000};
    uint64_t n_slots = 0;
    bmhip::DevBuf<uint8_t> in, skip;
    bmhip::DevBuf<uint64_t> rec_offset, d_ref_base;
    bmhip::DevBuf<uint32_t> d_ref_len, sites, calls;
    bmhip::DevBuf<unsigned long long> cell;
    float ms_add = 0.f, ms_call = 0.f;
};
