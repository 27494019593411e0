// mm_philox.h -- the counter-based generator of the sampling entries (mm_kernel_sample.hip, mm_kernel_latsample.hip): no generator
// state, so a draw depends on its key and its counter alone.
#pragma once
#include <hip/hip_runtime.h>

namespace mm {

// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011); the first two words
__device__ __forceinline__ uint2 philox_4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = unsigned(p1 >> 32) ^ c1 ^ k0, n2 = unsigned(p0 >> 32) ^ c3 ^ k1;
        c1 = unsigned(p1);
        c3 = unsigned(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint2(c0, c1);
}
// 23 random bits -> a uniform strictly inside (0, 1): (m + 1/2) / 2^23, exact in float32
__device__ __forceinline__ float unit_open(unsigned r) { return (float(r >> 9) + 0.5f) * 0x1p-23f; }

}  // namespace mm
