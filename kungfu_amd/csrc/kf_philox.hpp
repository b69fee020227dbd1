// kf_philox.hpp — the counter-based generator behind every stochastic rounding
// here (kf_adam_sr.hip; kf_mx8.hip's stochastic pack, §25):
// Philox2x32-10, and splitmix64 for the host side that turns a seed and a few
// indices into its key and counter words. Device code under __HIPCC__.
#pragma once
#include <cstdint>

namespace kf
{
// z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
// z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, modulo 2^64
inline uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#ifdef __HIPCC__
// Philox2x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
// 3"): ten rounds of {hi(M * c0) ^ key ^ c1, lo(M * c0)}, the key bumped by
// the golden ratio between rounds. The key sequence is wave-uniform.
struct Philox2 {
    uint32_t a, b;
};
// hi ^ key ^ c1 as one three-input bit operation where the target has one
// (truth table 0x96); key is wave-uniform.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
__device__ __forceinline__ Philox2 philox2x32_10(uint32_t c0, uint32_t c1, uint32_t key)
{
    constexpr uint32_t M = 0xD256D193u, W = 0x9E3779B9u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t prod = static_cast<uint64_t>(M) * c0;
        c0 = xor3(static_cast<uint32_t>(prod >> 32), key, c1);
        c1 = static_cast<uint32_t>(prod);
        key += W;
    }
    return Philox2{c0, c1};
}
#endif  // __HIPCC__

}  // namespace kf
