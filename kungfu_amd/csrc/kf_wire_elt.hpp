// kf_wire_elt.hpp — what the gradient wires' kernels share (kf_mx8.hip,
// kf_sign1.hip, kf_topk.hip): the pack's load of a lane's 8 elements, and the
// fold's epilogue over a lane's 16 or 4 f32 accumulators (/np, one narrowing,
// 16-byte stores). The formats and their cross-lane steps are each file's own.
#pragma once
#include "kf_sgd_elt.hpp"

namespace kf
{
// the lane's 8 elements, widened (exactly); zeros outside the shard
template <typename T>
__device__ __forceinline__ void wire_load8(const void *src, size_t u, bool active, float (&x)[8])
{
    u32x4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0};
    if constexpr (std::is_same<T, float>::value) {
        if (active) {
            r0 = ld_u4<1>(src, 2 * u);
            r1 = ld_u4<1>(src, 2 * u + 1);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i]     = __uint_as_float(r0[i]);
            x[4 + i] = __uint_as_float(r1[i]);
        }
    } else {
        if (active) r0 = ld_u4<1>(src, u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i]     = SgdElt<T>::widen(static_cast<uint16_t>(r0[i]));
            x[2 * i + 1] = SgdElt<T>::widen(static_cast<uint16_t>(r0[i] >> 16));
        }
    }
}

// the one narrowing of a finished f32 value: never fused with the operation
// that made it (kf_reduce_kernels.hpp f32_product_to_f16)
template <typename T> __device__ __forceinline__ uint16_t wire_narrow(float s)
{
    asm("" : "+v"(s));
    return SgdElt<T>::narrow(s);
}

// The fold's epilogue: unit u's 16 sums / np (DIV: SgdDiv's), narrowed once,
// stored as 4 x 16 bytes (f32) or 2 x 16 bytes (bf16, f16). Cached stores:
// the update kernel reads the shard next.
template <typename T, int DIV>
__device__ __forceinline__ void wire_store16(void *out, size_t u, float (&acc)[16], const Div &d)
{
    if constexpr (DIV != 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = SgdElt<float>::div<DIV == 1>(acc[i], d);
    }
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            st_u4<0>(out, 4 * u + w,
                     u32x4{__float_as_uint(acc[4 * w]), __float_as_uint(acc[4 * w + 1]),
                           __float_as_uint(acc[4 * w + 2]), __float_as_uint(acc[4 * w + 3])});
        }
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            u32x4 raw;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                raw[i] = static_cast<unsigned>(wire_narrow<T>(acc[8 * w + 2 * i])) |
                         (static_cast<unsigned>(wire_narrow<T>(acc[8 * w + 2 * i + 1])) << 16);
            }
            st_u4<0>(out, 2 * u + w, raw);
        }
    }
}

// The same epilogue over a lane's 4 sums (kf_topk.hip's read-out): unit u is
// 4 elements, stored as 16 bytes (f32) or 8 (bf16, f16).
typedef unsigned int wire_u32x2 __attribute__((ext_vector_type(2)));
template <typename T, int DIV>
__device__ __forceinline__ void wire_store4(void *out, size_t u, float (&acc)[4], const Div &d)
{
    if constexpr (DIV != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = SgdElt<float>::div<DIV == 1>(acc[i], d);
    }
    if constexpr (std::is_same<T, float>::value) {
        st_u4<0>(out, u,
                 u32x4{__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]),
                       __float_as_uint(acc[3])});
    } else {
        wire_u32x2 raw;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            raw[i] = static_cast<unsigned>(wire_narrow<T>(acc[2 * i])) |
                     (static_cast<unsigned>(wire_narrow<T>(acc[2 * i + 1])) << 16);
        }
        reinterpret_cast<wire_u32x2 *>(out)[u] = raw;
    }
}

}  // namespace kf
