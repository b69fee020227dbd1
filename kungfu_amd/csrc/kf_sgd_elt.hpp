// kf_sgd_elt.hpp — what the batched optimizer-update kernels share
// (kf_sgd.hip, kf_adam.hip, kf_adam_master.hip): the storage <-> compute
// traits of the four float dtypes, the /np of kf_bucket_div, and a 16-byte
// vector's unpack / pack.
#pragma once
#include "kf_reduce_kernels.hpp"

namespace kf
{
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Storage <-> compute. X is the compute scalar or a 2-lane vector of it:
// `*` and `+` are then one IEEE operation per lane (v_pk_mul_f32 /
// v_pk_add_f32 for fp32 pairs), and rnd() is the rounding to the storage type.
template <typename T> struct SgdElt;
template <> struct SgdElt<float> {
    using S = float;
    using C = float;
    using X = f32x2;
    __device__ static C widen(S s) { return s; }
    __device__ static S narrow(C c) { return c; }
    __device__ static C rnd(C c) { return c; }
    __device__ static X rnd(X x) { return x; }
    template <bool P2> __device__ static C div(C a, const Div &d)
    {
        return P2 ? __fmul_rn(a, d.fi) : __fdiv_rn(a, d.f);
    }
};
template <> struct SgdElt<double> {
    using S = double;
    using C = double;
    using X = f64x2;
    __device__ static C widen(S s) { return s; }
    __device__ static S narrow(C c) { return c; }
    __device__ static C rnd(C c) { return c; }
    __device__ static X rnd(X x) { return x; }
    template <bool P2> __device__ static C div(C a, const Div &d)
    {
        return P2 ? __dmul_rn(a, d.di) : __ddiv_rn(a, d.d);
    }
};
template <> struct SgdElt<f16_t> {
    using S = uint16_t;
    using C = float;
    using X = f32x2;
    __device__ static C widen(S s) { return f16_to_f32(s); }
    __device__ static S narrow(C c) { return f32_to_f16(c); }
    // rnd() is handed products: f32_product_to_f16 (kf_reduce_kernels.hpp)
    // keeps them from reaching the narrowing convert as a multiply, which
    // the compiler would select as v_fma_mixlo_f16 (x * y + 0): the +0
    // addend turns a -0 product into +0.
    __device__ static C rnd(C c) { return f16_to_f32(f32_product_to_f16(c)); }
    __device__ static X rnd(X x) { return X{rnd(x.x), rnd(x.y)}; }
    template <bool P2> __device__ static C div(C a, const Div &d)
    {
        return P2 ? __fmul_rn(a, d.fi) : __fdiv_rn(a, d.f);
    }
};
template <> struct SgdElt<bf16_t> {
    using S = uint16_t;
    using C = float;
    using X = f32x2;
    __device__ static C widen(S s) { return bf16_to_f32(s); }
    __device__ static S narrow(C c) { return f32_to_bf16(c); }
    __device__ static C rnd(C c) { return bf16_to_f32(f32_to_bf16(c)); }
    __device__ static X rnd(X x) { return X{rnd(x.x), rnd(x.y)}; }
    template <bool P2> __device__ static C div(C a, const Div &d)
    {
        return P2 ? __fmul_rn(a, d.fi) : __fdiv_rn(a, d.f);
    }
};

// DIV: 0 = no /np, 1 = multiply by 2^-k, 2 = true division
template <typename T, int DIV> struct SgdDiv {
    using E = SgdElt<T>;
    using C = typename E::C;
    using X = typename E::X;
    __device__ static C run(C g, const Div &d)
    {
        if constexpr (DIV == 0) return g;
        else return E::rnd(E::template div<DIV == 1>(g, d));
    }
    __device__ static X run(X g, const Div &d)
    {
        if constexpr (DIV == 0) {
            return g;
        } else if constexpr (DIV == 1) {
            const C inv = E::template div<true>(C(1), d);  // 2^-k, exact
            return E::rnd(g * inv);
        } else {
            return E::rnd(X{E::template div<false>(g.x, d), E::template div<false>(g.y, d)});
        }
    }
};

// a 16-B vector of storage elements <-> N/2 two-lane compute values
template <typename T> struct SgdVec {
    using E = SgdElt<T>;
    using S = typename E::S;
    using X = typename E::X;
    static constexpr int N = 16 / sizeof(S);
    __device__ static void unpack(const u32x4 &raw, X (&x)[N / 2])
    {
        if constexpr (std::is_same<T, bf16_t>::value) {
            // a 32-bit word holds two bf16 lanes: the low one widens by a
            // shift, the high one by a mask
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                x[w] = X{__uint_as_float(raw[w] << 16), __uint_as_float(raw[w] & 0xffff0000u)};
            }
        } else {
            Vec<S> v;
            __builtin_memcpy(&v, &raw, 16);
#pragma unroll
            for (int i = 0; i < N / 2; ++i) x[i] = X{E::widen(v.e[2 * i]), E::widen(v.e[2 * i + 1])};
        }
    }
    __device__ static u32x4 pack(const X (&x)[N / 2])
    {
        Vec<S> v;
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            v.e[2 * i]     = E::narrow(x[i].x);
            v.e[2 * i + 1] = E::narrow(x[i].y);
        }
        u32x4 raw;
        __builtin_memcpy(&raw, &v, 16);
        return raw;
    }
};

template <int NT> __device__ __forceinline__ void st_u4(void *base, size_t vi, const u32x4 &raw)
{
    u32x4 *p = reinterpret_cast<u32x4 *>(base) + vi;
    if constexpr (NT) __builtin_nontemporal_store(raw, p);
    else *p = raw;
}

// The /np operands of np ranks, as kf_capi.hip's make_div; np == 0 is never
// divided by.
inline Div update_div(int np)
{
    Div dv;
    dv.f    = static_cast<float>(np);
    dv.d    = static_cast<double>(np);
    dv.pow2 = np > 0 && (np & (np - 1)) == 0;
    dv.fi   = np > 0 ? 1.0f / dv.f : 0.0f;  // exact for powers of two
    dv.di   = np > 0 ? 1.0 / dv.d : 0.0;
    return dv;
}
// the kernels' `div` argument that goes with it: SgdDiv's DIV
inline int update_div_code(int np, const Div &dv) { return np == 0 ? 0 : (dv.pow2 ? 1 : 2); }

}  // namespace kf
