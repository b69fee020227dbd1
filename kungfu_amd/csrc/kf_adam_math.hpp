// kf_adam_math.hpp — what the two Adam / AdamW update kernels share
// (kf_adam.hip, kf_adam_master.hip): the segment's scalars, the correctly
// rounded sqrt and division, and the update itself. The arithmetic is
// kf_adam.hip's header comment, one IEEE operation per parenthesis.
#pragma once
#include <cmath>

#include "kf_sgd_elt.hpp"
#include "kungfu_amd.h"

namespace kf
{
enum { ADAM_NO_DECAY = 0, ADAM_L2 = 1, ADAM_DECOUPLED = 2 };

// Correctly rounded sqrt and division of the compute scalar or of a lane pair.
__device__ __forceinline__ float adam_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double adam_sqrt(double x) { return __dsqrt_rn(x); }
__device__ __forceinline__ float adam_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double adam_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ f32x2 adam_sqrt(f32x2 x) { return f32x2{sqrtf(x.x), sqrtf(x.y)}; }
__device__ __forceinline__ f64x2 adam_sqrt(f64x2 x)
{
    return f64x2{__dsqrt_rn(x.x), __dsqrt_rn(x.y)};
}
__device__ __forceinline__ f32x2 adam_div(f32x2 a, float b)
{
    return f32x2{__fdiv_rn(a.x, b), __fdiv_rn(a.y, b)};
}
__device__ __forceinline__ f64x2 adam_div(f64x2 a, double b)
{
    return f64x2{__ddiv_rn(a.x, b), __ddiv_rn(a.y, b)};
}
__device__ __forceinline__ f32x2 adam_div(f32x2 a, f32x2 b)
{
    return f32x2{__fdiv_rn(a.x, b.x), __fdiv_rn(a.y, b.y)};
}
__device__ __forceinline__ f64x2 adam_div(f64x2 a, f64x2 b)
{
    return f64x2{__ddiv_rn(a.x, b.x), __ddiv_rn(a.y, b.y)};
}

// What a gated kernel (include/kungfu_amd.h kf_adam_update_batch_gated) read
// from the step's gate and its group's step state, in the compute type C; the
// ungated kernels pass no gate at all.
struct AdamNoGate {
    static constexpr bool on = false;
};
template <typename C> struct AdamGate {
    static constexpr bool on = true;
    C mul, s2, nss;
};

// The block's gate words, or nothing to do: true when the step is skipped.
// Ordinary loads through kernel-argument pointers, wave-uniform. All of them
// are issued before skip is looked at: one memory latency after the kernel
// arguments', not one for skip and another for the scalars behind it.
template <typename C>
__device__ __forceinline__ bool adam_gate_load(const kf_step_gate *gate, const kf_step_state *st,
                                               AdamGate<C> &out)
{
    const int skip = gate->skip;
    out.mul        = static_cast<C>(gate->grad_mul);
    if constexpr (std::is_same<C, double>::value) {
        out.s2  = st->s2_f64;
        out.nss = st->nss_f64;
    } else {
        out.s2  = st->s2;
        out.nss = st->nss;
    }
    return skip != 0;
}

// s2 and nss of an update: the segment's own, or the gate's.
template <typename SEG>
__device__ __forceinline__ auto adam_s2(const SEG &h, const AdamNoGate &) -> decltype(h.s2)
{
    return h.s2;
}
template <typename SEG>
__device__ __forceinline__ auto adam_nss(const SEG &h, const AdamNoGate &) -> decltype(h.nss)
{
    return h.nss;
}
template <typename SEG, typename C>
__device__ __forceinline__ C adam_s2(const SEG &, const AdamGate<C> &gate)
{
    return gate.s2;
}
template <typename SEG, typename C>
__device__ __forceinline__ C adam_nss(const SEG &, const AdamGate<C> &gate)
{
    return gate.nss;
}

// The update of H values (V = C) or of H lane pairs (V = X); g holds the
// summed gradients on entry; h is the segment's kernarg entry (SEG: its
// members w, b1, c1, b2, c2, s2, eps, nss in T's compute type), whose scalars
// are wave-uniform. DECAY is the segment's choice, made once per block. A
// gate adds g = rnd(g * mul) after the /np and replaces h.s2 and h.nss.
template <typename T, int DIV, int DECAY, int H, typename V, typename SEG,
          typename GATE = AdamNoGate>
__device__ __forceinline__ void adam_math(V (&p)[H], V (&g)[H], V (&m)[H], V (&v)[H], const SEG &h,
                                          const Div &d, const GATE &gate = GATE{})
{
    using E = SgdElt<T>;
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = SgdDiv<T, DIV>::run(g[i], d);
    if constexpr (GATE::on) {
#pragma unroll
        for (int i = 0; i < H; ++i) g[i] = E::rnd(g[i] * gate.mul);
    }
    if constexpr (DECAY == ADAM_L2) {
#pragma unroll
        for (int i = 0; i < H; ++i) g[i] = E::rnd(g[i] + h.w * p[i]);
    } else if constexpr (DECAY == ADAM_DECOUPLED) {
#pragma unroll
        for (int i = 0; i < H; ++i) p[i] = E::rnd(h.w * p[i]);
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V t = h.b1 * m[i];
        m[i]      = E::rnd(t + h.c1 * g[i]);
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V t = E::rnd(h.b2 * v[i]);
        const V q = g[i] * g[i];
        v[i]      = E::rnd(t + h.c2 * q);
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V r = E::rnd(adam_sqrt(v[i]));
        const V e = E::rnd(adam_div(r, adam_s2(h, gate)));
        const V f = E::rnd(e + h.eps);
        const V u = adam_div(m[i], f);
        p[i]      = E::rnd(p[i] + adam_nss(h, gate) * u);
    }
}

// The segment's decay, chosen once per block: a choice inside the update would
// be made per vector, and in the scalar tail it kept p and g in scratch.
// f(std::integral_constant<int, DECAY>).
template <typename F> __device__ __forceinline__ void dispatch_decay(int decay, F &&f)
{
    if (decay == ADAM_NO_DECAY) f(std::integral_constant<int, ADAM_NO_DECAY>{});
    else if (decay == ADAM_L2) f(std::integral_constant<int, ADAM_L2>{});
    else f(std::integral_constant<int, ADAM_DECOUPLED>{});
}

// The scalars of a kernarg entry from the caller's hyperparameters: computed
// in double, cast once to the compute type C.
template <typename C, typename SEG> inline void adam_scalars(SEG &g, const kf_adam_hyper &h)
{
    g.decay = h.weight_decay == 0 ? ADAM_NO_DECAY : (h.decoupled ? ADAM_DECOUPLED : ADAM_L2);
    g.w     = static_cast<C>(h.decoupled ? 1.0 - h.lr * h.weight_decay : h.weight_decay);
    g.b1    = static_cast<C>(h.beta1);
    g.c1    = static_cast<C>(1.0 - h.beta1);
    g.b2    = static_cast<C>(h.beta2);
    g.c2    = static_cast<C>(1.0 - h.beta2);
    g.s2    = static_cast<C>(std::sqrt(h.bias_correction2));
    g.eps   = static_cast<C>(h.eps);
    g.nss   = static_cast<C>(-(h.lr / h.bias_correction1));
}

}  // namespace kf
