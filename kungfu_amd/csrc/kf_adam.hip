// kf_adam.hip — the Adam / AdamW update fused into the shard step of a
// synchronous exchange (include/kungfu_amd.h kf_adam_update_batch, DESIGN.md
// §14):
//
//   reduce-scatter(grads) -> [own shard: g/np, weight decay, m, v,
//                             p -= step * m / (sqrt(v) / s2 + eps)] -> all-gather(params)
//
// One batched element-wise launch over up to kAdamSeg segments of one dtype,
// kf_sgd.hip's shape with two state streams (the launch planner and the
// segment lookup are kf_update_batch.hpp's). Every segment has its own param /
// grad / exp_avg / exp_avg_sq pointers, its count and its scalars, all in the
// kernarg segment (lr and the bias corrections change every step). A segment
// reads g, p, m and v once and writes p, m and v once: 7 accesses per element.
//
// Arithmetic: torch.optim.Adam / AdamW's single-tensor path with m as two
// products and a sum (torch's lerp_ is one fused op), one IEEE operation per
// parenthesis, no contraction (the pragma of kf_reduce_kernels.hpp and the
// Makefile's -ffp-contract=off):
//
//   g = np > 0 ? sum / np : sum                (np a power of two: sum * 2^-k)
//   wd != 0, decoupled == 0 (Adam, L2):  g = g + (wd*p)
//   wd != 0, decoupled != 0 (AdamW):     p = dk*p              dk = 1 - lr*wd
//   m = (b1*m) + (c1*g)                        c1 = 1 - beta1
//   v = (b2*v) + (c2*(g*g))                    c2 = 1 - beta2
//   d = (sqrt(v) / s2) + eps                   s2 = sqrt(bias_correction2)
//   p = p + (nss*(m / d))                      nss = -(lr / bias_correction1)
//
// dk, c1, c2, s2 and nss are computed in double on the host and cast once to
// the compute type; the bias corrections 1 - beta^t come from the caller (no
// pow here or on the device). f32 / f64 round every operation in that type.
// bf16 computes in fp32 and rounds to bf16 where torch's tensor ops do: after
// the /np, after the L2 add or the decay multiply, after m (once), after
// b2*v, after the v add, after the sqrt, after the / s2, after the + eps and
// after the final add. The sqrt and both divisions are correctly rounded:
// sqrtf (not __fsqrt_rn, which is a bare v_sqrt_f32 here), __fdiv_rn,
// __dsqrt_rn, __ddiv_rn.
//
// f16 is refused: eps = 1e-8 rounds to 0 in f16, so every element with v == 0
// (bucket padding, a parameter that never had a gradient) would be 0 / 0.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_adam_math.hpp"  // the update itself, shared with kf_adam_master.hip
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal: kf_sgd.hip's measured
// one. g is dead after this kernel; p, m and v are read and written in place.
#ifndef KF_ADAM_G_NT
#define KF_ADAM_G_NT 1
#endif
#ifndef KF_ADAM_PMV_NT
#define KF_ADAM_PMV_NT 0
#endif
#ifndef KF_ADAM_ST_NT
#define KF_ADAM_ST_NT 0
#endif

namespace kf
{
constexpr int kAdamSeg   = 24;
constexpr int kAdamBlock = 256;
#ifndef KF_ADAM_UNROLL
#define KF_ADAM_UNROLL 4  // 16-B vectors per lane per stream per tile
#endif
constexpr int kAdamUnroll = KF_ADAM_UNROLL;

// C: the compute type (float for f32 / bf16, double for f64). One segment's
// entries sit together, as kf_sgd.hip's SgdSeg.
template <typename C> struct AdamSeg {
    void *p;
    const void *g;
    void *m, *v;
    size_t n;
    C w;  // ADAM_L2: weight_decay; ADAM_DECOUPLED: dk = 1 - lr*weight_decay
    C b1, c1, b2, c2, s2, eps, nss;
    int decay;
};
template <typename C> struct AdamBatchArgs {
    AdamSeg<C> seg[kAdamSeg];
    unsigned blk0[kAdamSeg + 1];  // the search table (1-D grids only)
    int nseg;
};
// kf_sgd.hip's SgdBatchArgs budget: an entry is 112 bytes for f64, so 24 of them
static_assert(sizeof(AdamBatchArgs<double>) + sizeof(Div) <= 3072, "kernarg budget");

// one vector: p, m and v updated and stored
template <typename T, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void adam_vec(void *pp, void *pm, void *pv, size_t vi, const u32x4 &rp,
                                         const u32x4 &rg, const u32x4 &rm, const u32x4 &rv,
                                         const AdamSeg<typename SgdElt<T>::C> &h, const Div &d,
                                         const GATE &gate = GATE{})
{
    using SV        = SgdVec<T>;
    using X         = typename SV::X;
    constexpr int H = SV::N / 2;
    X p[H], g[H], m[H], v[H];
    SV::unpack(rp, p);
    SV::unpack(rg, g);
    SV::unpack(rm, m);
    SV::unpack(rv, v);
    adam_math<T, DIV, DECAY, H, X>(p, g, m, v, h, d, gate);
    st_u4<KF_ADAM_ST_NT>(pp, vi, SV::pack(p));
    st_u4<KF_ADAM_ST_NT>(pm, vi, SV::pack(m));
    st_u4<KF_ADAM_ST_NT>(pv, vi, SV::pack(v));
}

// Block `blk` of `nblk` on one segment.
template <typename T, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void adam_body(const AdamSeg<typename SgdElt<T>::C> &h, const Div &d,
                                          size_t blk, size_t nblk, const GATE &gate = GATE{})
{
    using E         = SgdElt<T>;
    using S         = typename E::S;
    using C         = typename E::C;
    constexpr int N = SgdVec<T>::N;
    constexpr int U = kAdamUnroll, B = kAdamBlock;
    void *pp = h.p, *pm = h.m, *pv = h.v;
    const void *pg    = h.g;
    const size_t n    = h.n;
    const size_t nvec = n / N;

    // the scalar tail: fewer than N elements, on the segment's first block
    const size_t ti = nvec * N + threadIdx.x;
    if (blk == 0 && ti < n) {
        S *sp       = reinterpret_cast<S *>(pp);
        const S *sq = reinterpret_cast<const S *>(pg);
        S *sm       = reinterpret_cast<S *>(pm);
        S *sv       = reinterpret_cast<S *>(pv);
        C p[1] = {E::widen(sp[ti])}, g[1] = {E::widen(sq[ti])};
        C m[1] = {E::widen(sm[ti])}, v[1] = {E::widen(sv[ti])};
        adam_math<T, DIV, DECAY, 1, C>(p, g, m, v, h, d, gate);
        sp[ti] = E::narrow(p[0]);
        sm[ti] = E::narrow(m[0]);
        sv[ti] = E::narrow(v[0]);
    }

    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nvec + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        if (v0 + (U - 1) * B < nvec) {
            // full tile: every load issued before the first use
            u32x4 rp[U], rg[U], rm[U], rv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = ld_u4<KF_ADAM_G_NT>(pg, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ld_u4<KF_ADAM_PMV_NT>(pp, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rm[u] = ld_u4<KF_ADAM_PMV_NT>(pm, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rv[u] = ld_u4<KF_ADAM_PMV_NT>(pv, v0 + u * B);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                adam_vec<T, DIV, DECAY>(pp, pm, pv, v0 + u * B, rp[u], rg[u], rm[u], rv[u], h, d,
                                        gate);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t vi = v0 + u * B;
                if (vi >= nvec) break;
                const u32x4 rg = ld_u4<KF_ADAM_G_NT>(pg, vi), rp = ld_u4<KF_ADAM_PMV_NT>(pp, vi);
                const u32x4 rm = ld_u4<KF_ADAM_PMV_NT>(pm, vi), rv = ld_u4<KF_ADAM_PMV_NT>(pv, vi);
                adam_vec<T, DIV, DECAY>(pp, pm, pv, vi, rp, rg, rm, rv, h, d, gate);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kAdamBlock)
    adam_update_kernel(AdamBatchArgs<typename SgdElt<T>::C> a, Div np, int div)
{
    using C = typename SgdElt<T>::C;
    size_t blk, nblk;  // kf_update_batch.hpp's two grids
    const AdamSeg<C> &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk);
        });
    });
}

// adam_update_kernel under a step gate (include/kungfu_amd.h
// kf_adam_update_batch_gated): a skipped step returns before anything is
// loaded; otherwise grad_mul, s2 and nss come from device memory, the segments'
// own s2 and nss are not read.
template <typename T>
__global__ void __launch_bounds__(kAdamBlock)
    adam_update_gated_kernel(AdamBatchArgs<typename SgdElt<T>::C> a, Div np, int div,
                             const kf_step_gate *__restrict__ gate,
                             const kf_step_state *__restrict__ st)
{
    using C = typename SgdElt<T>::C;
    AdamGate<C> gt;
    if (adam_gate_load(gate, st, gt)) return;
    size_t blk, nblk;
    const AdamSeg<C> &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk, gt);
        });
    });
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail{"kf_adam_update_batch"};
constexpr UpdateFail fail_gated{"kf_adam_update_batch_gated"};

// gate == nullptr: hyper[b] is segment b's and the parent kernel runs; else
// the one hyper[0] is every segment's and the gated kernel runs.
template <typename T>
int launch_adam(void *const *params, const void *const *grads, void *const *ms, void *const *vs,
                const size_t *counts, int nb, int np, const kf_adam_hyper *hyper, hipStream_t s,
                const kf_step_gate *gate = nullptr, const kf_step_state *st = nullptr)
{
    using C       = typename SgdElt<T>::C;
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    return plan_update_batch<AdamBatchArgs<C>>(
        counts, nb, SgdVec<T>::N, static_cast<size_t>(kAdamBlock) * kAdamUnroll,
        [&](AdamSeg<C> &g, int b) {
            g.p = params[b];
            g.g = grads[b];
            g.m = ms[b];
            g.v = vs[b];
            g.n = counts[b];
            adam_scalars<C>(g, hyper[gate ? 0 : b]);
        },
        [&](unsigned gx, unsigned gy, const AdamBatchArgs<C> &a) {
            if (gate) {
                adam_update_gated_kernel<T><<<dim3(gx, gy), kAdamBlock, 0, s>>>(a, dv, div, gate, st);
                return launch_status(fail_gated);
            }
            adam_update_kernel<T><<<dim3(gx, gy), kAdamBlock, 0, s>>>(a, dv, div);
            return launch_status(fail);
        });
}

// Both entries: every check comes before any HIP call.
int adam_entry(const UpdateFail &fail, void *const *params, const void *const *grads,
               void *const *exp_avgs, void *const *exp_avg_sqs, const size_t *counts, int nb,
               KungFu_Datatype dt, int np, const kf_adam_hyper *hyper, UpdateGate *g, void *stream)
{
    const int rc = check_update_batch(
        fail, {{params, 16, kOff16}, {grads, 16, kOff16}, {exp_avgs, 16, kOff16},
               {exp_avg_sqs, 16, kOff16}},
        {}, counts, nb, np, hyper, g, false,
        [&]() -> int {
            if (dt == KungFu_FLOAT || dt == KungFu_DOUBLE || dt == KungFu_BFLOAT16) return KF_OK;
            return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE",
                        "f32, bf16 and f64 only (eps = 1e-8 is 0 in f16: 0 / 0 where v == 0)");
        },
        no_check, no_check);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s              = static_cast<hipStream_t>(stream);
    const kf_step_gate *gate   = g ? g->gate : nullptr;
    const kf_step_state *state = g ? g->state : nullptr;
    switch (dt) {
    case KungFu_FLOAT:
        return launch_adam<float>(params, grads, exp_avgs, exp_avg_sqs, counts, nb, np, hyper, s,
                                  gate, state);
    case KungFu_DOUBLE:
        return launch_adam<double>(params, grads, exp_avgs, exp_avg_sqs, counts, nb, np, hyper, s,
                                  gate, state);
    default:
        return launch_adam<bf16_t>(params, grads, exp_avgs, exp_avg_sqs, counts, nb, np, hyper, s,
                                  gate, state);
    }
}

}  // namespace

extern "C" {

int kf_adam_update_batch(void *const *params, const void *const *grads, void *const *exp_avgs,
                         void *const *exp_avg_sqs, const size_t *counts, int nb,
                         KungFu_Datatype dt, int np, const kf_adam_hyper *hyper, void *stream)
{
    return adam_entry(fail, params, grads, exp_avgs, exp_avg_sqs, counts, nb, dt, np, hyper, nullptr,
                      stream);
}

int kf_adam_update_batch_gated(void *const *params, const void *const *grads,
                               void *const *exp_avgs, void *const *exp_avg_sqs,
                               const size_t *counts, int nb, KungFu_Datatype dt, int np,
                               const kf_adam_hyper *hyper, const kf_step_gate *gate,
                               const kf_step_state *state, void *stream)
{
    UpdateGate g = {gate, state, {}};
    return adam_entry(fail_gated, params, grads, exp_avgs, exp_avg_sqs, counts, nb, dt, np, hyper,
                      &g, stream);
}

}  // extern "C"
