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

// The moments of H values (V = C) or H lane pairs (V = SgdElt<T>::X), T float
// or double: g holds the summed gradients on entry; m and v are updated, u is
// the update direction; p is only read. DECAY is the segment's choice, made
// once per block.
template <typename T, int DIV, int DECAY, int H, typename V, typename C>
__device__ __forceinline__ void lamb_math(const V (&p)[H], V (&g)[H], V (&m)[H], V (&v)[H],
                                          V (&u)[H], const LambScalars<C> &h, const Div &d)
{
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = SgdDiv<T, DIV>::run(g[i], d);
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
        const V e = adam_div(r, h.s2);
        const V f = e + h.eps;
        const V q = adam_div(m[i], f);
        u[i]      = h.rb1 * q;
        if constexpr (DECAY != 0) u[i] = u[i] + h.w * p[i];
    }
}

}  // namespace kf
