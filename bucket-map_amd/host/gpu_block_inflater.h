// gpu_block_inflater.h -- the product's bm::block_inflater: compressed -q and --genome are inflated by bmu_inflate
// (include/bmu.h) on one device.  No host fall-back: a failing device call ends the run.
#pragma once

#include "../../include/bmu.h"
#include "bgzf_in.h"

#include <stdexcept>
#include <string>

namespace bm {

class gpu_block_inflater : public block_inflater {
    int device_;
    bmu_ctx *ctx_ = nullptr;       // made by the first compressed file: a run on plain inputs pays nothing for it

public:
    explicit gpu_block_inflater(int device) : device_(device) {}
    ~gpu_block_inflater() override { bmu_destroy(ctx_); }
    gpu_block_inflater(const gpu_block_inflater &) = delete;
    gpu_block_inflater &operator=(const gpu_block_inflater &) = delete;

    uint64_t inflate(const uint8_t *in, size_t n, uint8_t *out, size_t out_cap) override {
        if (!ctx_ && bmu_create(device_, &ctx_) != BMU_OK) throw std::runtime_error(std::string("bmu_create: ") + bmu_last_error());
        uint64_t got = 0;
        if (bmu_inflate(ctx_, in, n, out, out_cap, &got) != BMU_OK) throw std::runtime_error(std::string("bmu_inflate: ") + bmu_last_error());
        return got;
    }
};

}  // namespace bm
