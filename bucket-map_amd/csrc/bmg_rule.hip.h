// bmg_rule.hip.h -- what the kernels of bmg_kernels.hip.h and of bmr_kernels.hip.h share of the genotype rule (include/bmg.h):
// the constants, the parameters and the ten costs of one position.  It defines no kernel, so several translation units of
// libbmf.so may include it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmg {

constexpr uint32_t kCells = 4, kGenotypes = 10;          // BMG_N_CELLS, BMG_N_GENOTYPES
constexpr uint64_t kU32Max = 0xFFFFFFFFull;

struct params {
    uint32_t min_mapq, min_bq, q_absent, q_cap, prior;
};

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > kU32Max ? (uint32_t)kU32Max : (uint32_t)v; }

// L[k] = L'(g) of the ten genotypes k = b (b + 1) / 2 + a from one position's n and Q, in u64 registers: everything is indexed
// by unrolled counters.  call_kernel and bmr's conf_kernel (with the prior 0, which makes it L) share it.
__device__ __forceinline__ void costs(const uint64_t (&n)[4], const uint64_t (&Q)[4], uint32_t R, uint32_t prior, uint64_t (&L)[kGenotypes]) {
    uint64_t M[4], T[4], all = 0;
#pragma unroll
    for (uint32_t a = 0; a < 4; a++) {
        M[a] = 100u * Q[a] + 477u * n[a];                // < 2^42
        T[a] = 301u * n[a];
        all += M[a];
    }
    uint32_t k = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
#pragma unroll
        for (uint32_t a = 0; a <= b; a++, k++) {
            const uint64_t like = a == b ? all - M[a] : T[a] + T[b] + all - M[a] - M[b];
            const uint32_t others = (a != R ? 1u : 0u) + (b != R && b != a ? 1u : 0u);
            L[k] = like + (uint64_t)prior * others;
        }
}

}  // namespace bmg
