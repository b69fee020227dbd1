// kf_lamb_math.hpp — the arithmetic of the LAMB moments pass, shared by the
// two moments kernels of kf_lamb.hip (f32 / f64 parameters, and 16-bit
// parameters through their fp32 master copy). The definition is
// include/kungfu_amd.h's ("LAMB"), one IEEE operation per parenthesis; the
// correctly rounded sqrt and divisions are kf_adam_math.hpp's.
#pragma once
#include <cmath>

#include "kf_adam_math.hpp"

namespace kf
{
// A segment's scalars in the compute type C, at the end of its kernarg entry.
template <typename C> struct LambScalars {
    C w;  // weight_decay (LAMB's lambda)
    C b1, c1, b2, c2, s2, eps, rb1;
    int decay;  // weight_decay != 0
};

// Computed in double, cast once to the compute type C (adam_scalars' rule).
// lr and decoupled are not looked at.
template <typename C> inline void lamb_scalars(LambScalars<C> &k, const kf_adam_hyper &h)
{
    k.decay = h.weight_decay != 0;
    k.w     = static_cast<C>(h.weight_decay);
    k.b1    = static_cast<C>(h.beta1);
    k.c1    = static_cast<C>(1.0 - h.beta1);
    k.b2    = static_cast<C>(h.beta2);
    k.c2    = static_cast<C>(1.0 - h.beta2);
    k.s2    = static_cast<C>(std::sqrt(h.bias_correction2));
    k.eps   = static_cast<C>(h.eps);
    k.rb1   = static_cast<C>(1.0 / h.bias_correction1);
}

// s2 and rb1 of a moments pass: the segment's own, or the gate's (kf_adam_math.hpp's
// AdamGate<C>, read by adam_gate_load). The gate's step state was advanced with
// lr = 1, so its nss is -(1 / (1 - beta1_pow)) and rb1 = -nss, exactly.
template <typename C> __device__ __forceinline__ C lamb_s2(const LambScalars<C> &h, const AdamNoGate &)
{
    return h.s2;
}
template <typename C> __device__ __forceinline__ C lamb_rb1(const LambScalars<C> &h, const AdamNoGate &)
{
    return h.rb1;
}
template <typename C> __device__ __forceinline__ C lamb_s2(const LambScalars<C> &, const AdamGate<C> &gate)
{
    return gate.s2;
}
template <typename C> __device__ __forceinline__ C lamb_rb1(const LambScalars<C> &, const AdamGate<C> &gate)
{
    return -gate.nss;
}

// The moments of H values (V = C) or H lane pairs (V = SgdElt<T>::X), T float
// or double: g holds the summed gradients on entry; m and v are updated, u is
// the update direction; p is only read. DECAY is the segment's choice, made
// once per block. A gate adds g = (g * mul) after the /np and replaces h.s2
// and h.rb1 (include/kungfu_amd.h "LAMB under a gate").
template <typename T, int DIV, int DECAY, int H, typename V, typename C,
          typename GATE = AdamNoGate>
__device__ __forceinline__ void lamb_math(const V (&p)[H], V (&g)[H], V (&m)[H], V (&v)[H],
                                          V (&u)[H], const LambScalars<C> &h, const Div &d,
                                          const GATE &gate = GATE{})
{
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = SgdDiv<T, DIV>::run(g[i], d);
    if constexpr (GATE::on) {
#pragma unroll
        for (int i = 0; i < H; ++i) g[i] = g[i] * gate.mul;
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V t = h.b1 * m[i];
        m[i]      = t + h.c1 * g[i];
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V t = h.b2 * v[i];
        const V q = g[i] * g[i];
        v[i]      = t + h.c2 * q;
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V r = adam_sqrt(v[i]);
        const V e = adam_div(r, lamb_s2(h, gate));
        const V f = e + h.eps;
        const V q = adam_div(m[i], f);
        u[i]      = lamb_rb1(h, gate) * q;
        if constexpr (DECAY != 0) u[i] = u[i] + h.w * p[i];
    }
}

}  // namespace kf
