// kf_sgd.hip — the SGD update fused into the shard step of a synchronous
// exchange (include/kungfu_amd.h kf_sgd_update_batch):
//
//   reduce-scatter(grads) -> [own shard: g/np, weight decay, momentum,
//                             p -= lr*g] -> all-gather(params)
//
// One batched element-wise launch over up to kSgdSeg segments of one dtype.
// Every segment has its own param / grad / momentum pointers, its count and
// its hyperparameters; all of that sits in the kernarg segment (lr changes
// every step, so there is no device table to copy). A segment reads g, p and
// m once and writes p and m once: 5 accesses per element (3 without momentum,
// 4 on a group's first step, which does not read m).
//
// Arithmetic: torch.optim.SGD's single-tensor path, one IEEE operation per
// step, no contraction (the pragma of kf_reduce_kernels.hpp and the
// Makefile's -ffp-contract=off):
//
//   g = np > 0 ? sum / np : sum       (np a power of two: sum * 2^-k)
//   if wd != 0:  g = g + wd*p
//   if mu != 0:  m = first ? g : (mu*m) + (c*g)        c = 1 - dampening
//                g = nesterov ? g + mu*m : m
//   p = p + nlr*g                                      nlr = -lr
//
// f32 / f64 round every product and every sum in that type. f16 / bf16
// compute in fp32 and round to the storage type where torch's tensor ops do:
// after the /np, after the weight-decay add, after mu*m, after the momentum
// add, after the nesterov add and after the final add; inside each of those
// ops the alpha*x product and the add are two fp32 roundings.
//
// Shape: kf_reduce_kernels.hpp's batched kernels. One 256-thread block per
// tile of 4 x 256 16-B vectors; all of a tile's loads (up to 12 per lane) are
// issued before the arithmetic. Segments of about equal size are the rows of
// a 2-D grid, others share a 1-D grid through a search table
// (kf_update_batch.hpp's planner, which the Adam kernels use too). Every pointer
// is 16-byte aligned (the host checks it), so a segment is whole vectors and
// a scalar tail of fewer than 16 bytes; there is no head.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_sgd_elt.hpp"
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal. g is dead after this
// kernel and is read non-temporally; p and m are read and then written in
// place, p is read next by the all-gather and m by the next step, and both go
// plain. ResNet-50's 25.6 M fp32 in 16 segments, kernel time from a kernel
// trace, as a fraction of 8 TB/s (5 accesses per element; the SMA blend of
// the same run beside it): all three non-temporal 0.680 (blend 0.793), plain
// stores 0.740 (0.787), plain stores and plain p / m loads 0.768 (0.820);
// event-timed, everything plain 0.676 against 0.720 for the shipped policy
// (tools/bench_sharded_sgd.py, profiles/sharded_sgd/ab_policy*.jsonl).
// Two vectors per lane per stream instead of four: 0.606 against 0.647.
#ifndef KF_SGD_G_NT
#define KF_SGD_G_NT 1
#endif
#ifndef KF_SGD_PM_NT
#define KF_SGD_PM_NT 0
#endif
#ifndef KF_SGD_ST_NT
#define KF_SGD_ST_NT 0
#endif

namespace kf
{
constexpr int kSgdSeg    = 32;
constexpr int kSgdBlock  = 256;
#ifndef KF_SGD_UNROLL
#define KF_SGD_UNROLL 4  // 16-B vectors per lane per stream per tile
#endif
constexpr int kSgdUnroll = KF_SGD_UNROLL;

enum { SGD_NESTEROV = 1, SGD_FIRST = 2 };

// C: the compute type (float for f32 / f16 / bf16, double for f64).
// One segment's entries sit together (one or two 64-byte lines of the kernarg
// segment): a block reads them with one round of scalar loads. As separate
// arrays they were nine lines per segment, and a launch over 16 segments
// carried about 24 us that did not depend on its size (ResNet-50's shard
// form, 64 MB of traffic, 36 us; tools/bench_sharded_sgd.py,
// profiles/sharded_sgd/ab_layout.jsonl).
template <typename C> struct SgdSeg {
    void *p;
    const void *g;
    void *m;  // NULL: no momentum stream (mu == 0)
    size_t n;
    C nlr, mu, c, wd;
    int flags;
};
template <typename C> struct SgdBatchArgs {
    SgdSeg<C> seg[kSgdSeg];
    unsigned blk0[kSgdSeg + 1];  // the search table (1-D grids only)
    int nseg;
};
static_assert(sizeof(SgdBatchArgs<double>) + sizeof(Div) <= 3072, "kernarg budget");

// one segment's scalars, read once per block (wave-uniform)
template <typename C> struct SgdHyper {
    C nlr, mu, c, wd;
    bool has_m, first, nesterov;
};

// The update of H values (V = C) or of H lane pairs (V = X); g holds the
// summed gradients on entry. Stage by stage over the H values, so that each
// choice (on the segment's scalars: wave-uniform) is one branch per vector
// and not one per element.
template <typename T, int DIV, int H, typename V>
__device__ __forceinline__ void sgd_math(V (&p)[H], V (&g)[H], V (&m)[H],
                                         const SgdHyper<typename SgdElt<T>::C> &h, const Div &d)
{
    using E = SgdElt<T>;
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = SgdDiv<T, DIV>::run(g[i], d);
    if (h.wd != 0) {
#pragma unroll
        for (int i = 0; i < H; ++i) g[i] = E::rnd(g[i] + h.wd * p[i]);
    }
    if (h.has_m) {
        if (h.first) {
#pragma unroll
            for (int i = 0; i < H; ++i) m[i] = g[i];
        } else {
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const V t = E::rnd(h.mu * m[i]);
                m[i]      = E::rnd(t + h.c * g[i]);
            }
        }
        if (h.nesterov) {
#pragma unroll
            for (int i = 0; i < H; ++i) g[i] = E::rnd(g[i] + h.mu * m[i]);
        } else {
#pragma unroll
            for (int i = 0; i < H; ++i) g[i] = m[i];
        }
    }
#pragma unroll
    for (int i = 0; i < H; ++i) p[i] = E::rnd(p[i] + h.nlr * g[i]);
}

// one vector: p and m updated and stored
template <typename T, int DIV>
__device__ __forceinline__ void sgd_vec(void *pp, void *pm, size_t vi, const u32x4 &rp,
                                        const u32x4 &rg, const u32x4 &rm,
                                        const SgdHyper<typename SgdElt<T>::C> &h, const Div &d)
{
    using SV        = SgdVec<T>;
    using X         = typename SV::X;
    constexpr int H = SV::N / 2;
    X p[H], g[H], m[H];
    SV::unpack(rp, p);
    SV::unpack(rg, g);
    SV::unpack(rm, m);
    sgd_math<T, DIV, H, X>(p, g, m, h, d);
    st_u4<KF_SGD_ST_NT>(pp, vi, SV::pack(p));
    if (h.has_m) st_u4<KF_SGD_ST_NT>(pm, vi, SV::pack(m));
}

// Block `blk` of `nblk` on one segment.
template <typename T, int DIV>
__device__ __forceinline__ void sgd_body(void *pp, const void *pg, void *pm, size_t n,
                                         const SgdHyper<typename SgdElt<T>::C> &h, const Div &d,
                                         size_t blk, size_t nblk)
{
    using E         = SgdElt<T>;
    using S         = typename E::S;
    using C         = typename E::C;
    constexpr int N = SgdVec<T>::N;
    constexpr int U = kSgdUnroll, B = kSgdBlock;
    const size_t nvec = n / N;
    const bool ld_m   = h.has_m && !h.first;  // a first step never reads m

    // the scalar tail: fewer than N elements, on the segment's first block
    const size_t ti = nvec * N + threadIdx.x;
    if (blk == 0 && ti < n) {
        S *sp       = reinterpret_cast<S *>(pp);
        const S *sg = reinterpret_cast<const S *>(pg);
        S *sm       = reinterpret_cast<S *>(pm);
        C p[1] = {E::widen(sp[ti])}, g[1] = {E::widen(sg[ti])};
        C m[1] = {ld_m ? E::widen(sm[ti]) : C(0)};
        sgd_math<T, DIV, 1, C>(p, g, m, h, d);
        sp[ti] = E::narrow(p[0]);
        if (h.has_m) sm[ti] = E::narrow(m[0]);
    }

    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nvec + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        if (v0 + (U - 1) * B < nvec) {
            // full tile: every load issued before the first use
            u32x4 rp[U], rg[U], rm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = ld_u4<KF_SGD_G_NT>(pg, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ld_u4<KF_SGD_PM_NT>(pp, v0 + u * B);
            if (ld_m) {
#pragma unroll
                for (int u = 0; u < U; ++u) rm[u] = ld_u4<KF_SGD_PM_NT>(pm, v0 + u * B);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) rm[u] = u32x4{0, 0, 0, 0};
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sgd_vec<T, DIV>(pp, pm, v0 + u * B, rp[u], rg[u], rm[u], h, d);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t vi = v0 + u * B;
                if (vi >= nvec) break;
                const u32x4 rg = ld_u4<KF_SGD_G_NT>(pg, vi), rp = ld_u4<KF_SGD_PM_NT>(pp, vi);
                const u32x4 rm = ld_m ? ld_u4<KF_SGD_PM_NT>(pm, vi) : u32x4{0, 0, 0, 0};
                sgd_vec<T, DIV>(pp, pm, vi, rp, rg, rm, h, d);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kSgdBlock)
    sgd_update_kernel(SgdBatchArgs<typename SgdElt<T>::C> a, Div np, int div)
{
    using C = typename SgdElt<T>::C;
    // kf_update_batch.hpp's batch_segment and, below, its dispatch_div, both
    // written out: through the helpers this kernel's code does not stay the
    // same (the Adam kernels' does).
    const bool rows = gridDim.y > 1;
    int s           = static_cast<int>(blockIdx.y);
    size_t blk = blockIdx.x, nblk = gridDim.x;
    if (!rows) {
        const unsigned b = blockIdx.x;
        int lo = 0, hi = a.nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (b >= a.blk0[mid]) lo = mid;
            else hi = mid - 1;
        }
        s    = lo;
        blk  = b - a.blk0[s];
        nblk = a.blk0[s + 1] - a.blk0[s];
    }
    const SgdSeg<C> &g = a.seg[s];
    SgdHyper<C> h;
    h.nlr      = g.nlr;
    h.mu       = g.mu;
    h.c        = g.c;
    h.wd       = g.wd;
    h.has_m    = g.m != nullptr;
    h.first    = (g.flags & SGD_FIRST) != 0;
    h.nesterov = (g.flags & SGD_NESTEROV) != 0;
    // the /np choice made once per kernel (kf_reduce_kernels.hpp EPI_MUL)
    if (div == 0) sgd_body<T, 0>(g.p, g.g, g.m, g.n, h, np, blk, nblk);
    else if (div == 1) sgd_body<T, 1>(g.p, g.g, g.m, g.n, h, np, blk, nblk);
    else sgd_body<T, 2>(g.p, g.g, g.m, g.n, h, np, blk, nblk);
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail{"kf_sgd_update_batch"};

template <typename T>
int launch_sgd(void *const *params, const void *const *grads, void *const *moms,
               const size_t *counts, int nb, int np, const kf_sgd_hyper *hyper, hipStream_t s)
{
    using C       = typename SgdElt<T>::C;
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    return plan_update_batch<SgdBatchArgs<C>>(
        counts, nb, SgdVec<T>::N, static_cast<size_t>(kSgdBlock) * kSgdUnroll,
        [&](SgdSeg<C> &g, int b) {
            const kf_sgd_hyper &h = hyper[b];
            g.p                   = params[b];
            g.g                   = grads[b];
            g.m                   = h.momentum != 0 ? moms[b] : nullptr;
            g.n                   = counts[b];
            // computed in double, cast once to the compute type
            g.nlr   = static_cast<C>(-h.lr);
            g.mu    = static_cast<C>(h.momentum);
            g.c     = static_cast<C>(1.0 - h.dampening);
            g.wd    = static_cast<C>(h.weight_decay);
            g.flags = (h.nesterov ? SGD_NESTEROV : 0) | (h.first ? SGD_FIRST : 0);
        },
        [&](unsigned gx, unsigned gy, const SgdBatchArgs<C> &a) {
            sgd_update_kernel<T><<<dim3(gx, gy), kSgdBlock, 0, s>>>(a, dv, div);
            return launch_status(fail);
        });
}

}  // namespace

extern "C" {

int kf_sgd_update_batch(void *const *params, const void *const *grads, void *const *moms,
                        const size_t *counts, int nb, KungFu_Datatype dt, int np,
                        const kf_sgd_hyper *hyper, void *stream)
{
    if (nb < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "nb < 0");
    if (nb == 0) return KF_OK;
    if (!params || !grads || !counts || !hyper) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    if (dt != KungFu_FLOAT && dt != KungFu_DOUBLE && dt != KungFu_FLOAT16 && dt != KungFu_BFLOAT16) {
        return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "f32, f16, bf16 and f64 only");
    }
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] == 0) continue;
        void *m = moms ? moms[b] : nullptr;
        if (!params[b] || !grads[b]) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty segment");
        }
        if (hyper[b].momentum != 0 && !m) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "momentum != 0 needs a momentum buffer");
        }
        if (off16(params[b]) || off16(grads[b]) || off16(m)) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "pointers must be 16-byte aligned");
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dt) {
    case KungFu_FLOAT: return launch_sgd<float>(params, grads, moms, counts, nb, np, hyper, s);
    case KungFu_DOUBLE: return launch_sgd<double>(params, grads, moms, counts, nb, np, hyper, s);
    case KungFu_FLOAT16: return launch_sgd<f16_t>(params, grads, moms, counts, nb, np, hyper, s);
    default: return launch_sgd<bf16_t>(params, grads, moms, counts, nb, np, hyper, s);
    }
}

}  // extern "C"
