// kf_lamb.hip — LAMB on the sharded step (include/kungfu_amd.h "LAMB",
// DESIGN.md §17): layer-wise trust ratios where a tensor's elements are spread
// over the ranks' shards.
//
//   reduce-scatter(grads) -> [own shard: moments: m, v, u]
//                         -> segmented norms of (p, u) pieces, all-gather of the sums
//                         -> trust: nlr[t] = -(lr_t * ratio_t)
//                         -> [own pieces: p += nlr[t] * u] -> all-gather(params)
//
// Three kinds of kernel:
//   * the moments pass (lamb_moments_kernel, lamb_master_moments_kernel):
//     kf_adam.hip's shape, one batched launch over up to kLambSeg shard
//     segments through kf_update_batch.hpp's planner, 16-byte aligned
//     pointers and scalars in the kernarg segment. It reads g, p, m, v and
//     writes m, v and the update direction u: 7 accesses per element, 28 B for
//     f32, 26 B on the master path (g is 2 B there);
//   * the trust ratios (lamb_trust_kernel): one lane per tensor, fp64;
//   * the apply pass (lamb_apply_kernel, lamb_master_apply_kernel): a plan
//     like kf_segnorm.hip's over "tensor ∩ own shard" pieces, whose table
//     lives in HBM: one launch whatever the number of pieces. Pieces are
//     aligned to the element only: a scalar head up to the first index at
//     which every array of the piece is 16-byte aligned, vector tiles, a
//     scalar tail.
//
// The arithmetic is kf_lamb_math.hpp's, one IEEE operation per parenthesis, no
// contraction (the pragma of kf_reduce_kernels.hpp and -ffp-contract=off).
//
// Every kernel has a sibling under a step gate (include/kungfu_amd.h "LAMB
// under a gate"), lamb_*_gated_kernel, which reads the verdict
// of kf_step_gate.hip from device memory: a skipped step returns before it
// touches anything, an applied one multiplies the gradient by grad_mul after
// the /np and takes s2 and rb1 from the group's step state. They run the
// parents' bodies; the parents' device code does not change with them.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_lamb_math.hpp"
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal; the measured one
// (DESIGN.md §17). Moments: g is dead after the kernel; p is only read here;
// m and v are read and written in place; u is written only. Apply: u is dead
// after the kernel, p is read and written in place.
#ifndef KF_LAMB_P_NT
#define KF_LAMB_P_NT 1
#endif
#ifndef KF_LAMB_MV_NT
#define KF_LAMB_MV_NT 1
#endif
#ifndef KF_LAMB_U_NT
#define KF_LAMB_U_NT 1
#endif
#ifndef KF_LAMB_APPLY_P_NT
#define KF_LAMB_APPLY_P_NT 1
#endif
#ifndef KF_LAMB_APPLY_ST_NT
#define KF_LAMB_APPLY_ST_NT 0
#endif
// The apply pass: 16-byte units per lane per tile, and tiles per block.
#ifndef KF_LAMB_APPLY_UNROLL
#define KF_LAMB_APPLY_UNROLL 4
#endif
#ifndef KF_LAMB_APPLY_TILES
#define KF_LAMB_APPLY_TILES 1
#endif

namespace kf
{
constexpr int kLambSeg       = 24;  // f32 / f64 segments per launch (an f64 entry is 120 bytes)
constexpr int kLambMasterSeg = 32;  // master path: an entry is 88 bytes
constexpr int kLambBlock     = 256;
constexpr int kLambUnroll    = 4;  // 16-byte units of the compute type per lane per tile
constexpr int kTrustGroups   = 16;  // param groups per trust launch
constexpr int kApplyUnroll   = KF_LAMB_APPLY_UNROLL;
constexpr int kApplyTiles    = KF_LAMB_APPLY_TILES;

template <typename C> struct LambSeg {
    const void *p;  // parameters (or the fp32 master), read only
    const void *g;  // summed gradients, the parameters' storage type
    void *m, *v;    // exp_avg, exp_avg_sq
    void *u;        // the update direction, written only
    size_t n;
    LambScalars<C> k;
};
template <typename C, int NSEG> struct LambArgs {
    LambSeg<C> seg[NSEG];
    unsigned blk0[NSEG + 1];  // the search table (1-D grids only)
    int nseg;
};
static_assert(sizeof(LambArgs<double, kLambSeg>) + sizeof(Div) <= 3072, "kernarg budget");
static_assert(sizeof(LambArgs<float, kLambMasterSeg>) + sizeof(Div) <= 3072, "kernarg budget");
// the gated kernels: div, padding and the gate and step-state pointers behind it
static_assert(sizeof(LambArgs<double, kLambSeg>) + sizeof(Div) + 8 + 2 * sizeof(void *) <= 3072,
              "kernarg budget, gated");
static_assert(sizeof(LambArgs<float, kLambMasterSeg>) + sizeof(Div) + 8 + 2 * sizeof(void *) <= 3072,
              "kernarg budget, gated");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// The gradient stream of a unit (16 bytes of the compute type C): G == C reads
// 16 bytes, a 16-bit G reads 8 bytes and widens (exactly).
template <typename C, typename G> struct LambGrad {  // G: bf16_t or f16_t, C: float
    using R = u32x2;
    using X = f32x2;
    __device__ static R ld(const void *g, size_t ui)
    {
        return __builtin_nontemporal_load(reinterpret_cast<const R *>(g) + ui);
    }
    __device__ static X widen2(unsigned w)
    {
        if constexpr (std::is_same<G, bf16_t>::value) {
            return X{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
        } else {
            return X{SgdElt<G>::widen(static_cast<uint16_t>(w)),
                     SgdElt<G>::widen(static_cast<uint16_t>(w >> 16))};
        }
    }
    __device__ static void unpack(const R &r, X (&x)[2])
    {
        x[0] = widen2(r[0]);
        x[1] = widen2(r[1]);
    }
    __device__ static C scalar(const void *g, size_t i)
    {
        return SgdElt<G>::widen(reinterpret_cast<const uint16_t *>(g)[i]);
    }
};
template <typename C> struct LambGrad<C, C> {
    using R = u32x4;
    using X = typename SgdElt<C>::X;
    __device__ static R ld(const void *g, size_t ui) { return ld_u4<1>(g, ui); }
    __device__ static void unpack(const R &r, X (&x)[SgdVec<C>::N / 2]) { SgdVec<C>::unpack(r, x); }
    __device__ static C scalar(const void *g, size_t i) { return reinterpret_cast<const C *>(g)[i]; }
};

// one unit: m, v and u stored
template <typename C, typename G, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void lamb_unit(const LambSeg<C> &h, const Div &d, size_t ui,
                                          const typename LambGrad<C, G>::R &rg, const u32x4 &rp,
                                          const u32x4 &rm, const u32x4 &rv,
                                          const GATE &gate = GATE{})
{
    using SV        = SgdVec<C>;
    using X         = typename SV::X;
    constexpr int H = SV::N / 2;
    X p[H], g[H], m[H], v[H], u[H];
    LambGrad<C, G>::unpack(rg, g);
    SV::unpack(rp, p);
    SV::unpack(rm, m);
    SV::unpack(rv, v);
    lamb_math<C, DIV, DECAY, H, X>(p, g, m, v, u, h.k, d, gate);
    st_u4<0>(h.m, ui, SV::pack(m));
    st_u4<0>(h.v, ui, SV::pack(v));
    st_u4<KF_LAMB_U_NT>(h.u, ui, SV::pack(u));
}

// Block `blk` of `nblk` on one segment.
template <typename C, typename G, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void lamb_body(const LambSeg<C> &h, const Div &d, size_t blk, size_t nblk,
                                          const GATE &gate = GATE{})
{
    using LG        = LambGrad<C, G>;
    constexpr int N = SgdVec<C>::N;
    constexpr int U = kLambUnroll, B = kLambBlock;
    const size_t n     = h.n;
    const size_t nunit = n / N;

    // the scalar tail: fewer than N elements, on the segment's first block
    const size_t ti = nunit * N + threadIdx.x;
    if (blk == 0 && ti < n) {
        const C *sp = reinterpret_cast<const C *>(h.p);
        C *sm = reinterpret_cast<C *>(h.m), *sv = reinterpret_cast<C *>(h.v);
        C *su = reinterpret_cast<C *>(h.u);
        const C p[1] = {sp[ti]};
        C g[1] = {LG::scalar(h.g, ti)}, m[1] = {sm[ti]}, v[1] = {sv[ti]}, u[1];
        lamb_math<C, DIV, DECAY, 1, C>(p, g, m, v, u, h.k, d, gate);
        sm[ti] = m[0];
        sv[ti] = v[0];
        su[ti] = u[0];
    }

    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nunit + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u0 = t * tile + threadIdx.x;
        if (u0 + (U - 1) * B < nunit) {
            // full tile: every load issued before the first use
            typename LG::R rg[U];
            u32x4 rp[U], rm[U], rv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = LG::ld(h.g, u0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ld_u4<KF_LAMB_P_NT>(h.p, u0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rm[u] = ld_u4<KF_LAMB_MV_NT>(h.m, u0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rv[u] = ld_u4<KF_LAMB_MV_NT>(h.v, u0 + u * B);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                lamb_unit<C, G, DIV, DECAY>(h, d, u0 + u * B, rg[u], rp[u], rm[u], rv[u], gate);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t ui = u0 + u * B;
                if (ui >= nunit) break;
                const typename LG::R rg = LG::ld(h.g, ui);
                const u32x4 rp = ld_u4<KF_LAMB_P_NT>(h.p, ui), rm = ld_u4<KF_LAMB_MV_NT>(h.m, ui),
                            rv = ld_u4<KF_LAMB_MV_NT>(h.v, ui);
                lamb_unit<C, G, DIV, DECAY>(h, d, ui, rg, rp, rm, rv, gate);
            }
        }
    }
}

template <typename C, typename G, typename ARGS, typename GATE = AdamNoGate>
__device__ __forceinline__ void lamb_moments(const ARGS &a, const Div &np, int div,
                                             const GATE &gate = GATE{})
{
    size_t blk, nblk;  // kf_update_batch.hpp's two grids
    const LambSeg<C> &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        if (g.k.decay) lamb_body<C, G, decltype(DIV)::value, 1>(g, np, blk, nblk, gate);
        else lamb_body<C, G, decltype(DIV)::value, 0>(g, np, blk, nblk, gate);
    });
}

// T: float or double, the parameters' own type
template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_moments_kernel(LambArgs<T, kLambSeg> a, Div np, int div)
{
    lamb_moments<T, T>(a, np, div);
}

// T: bf16_t or f16_t, the gradients' storage type; everything else is fp32
template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_master_moments_kernel(LambArgs<float, kLambMasterSeg> a, Div np, int div)
{
    lamb_moments<float, T>(a, np, div);
}

// The moments pass under a step gate (include/kungfu_amd.h "LAMB under a
// gate"): a skipped step returns before anything is loaded; otherwise grad_mul,
// s2 and rb1 = -nss come from device memory, the segments' own s2 and rb1 are
// not read.
template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_moments_gated_kernel(LambArgs<T, kLambSeg> a, Div np, int div,
                              const kf_step_gate *__restrict__ gate,
                              const kf_step_state *__restrict__ st)
{
    AdamGate<T> gt;
    if (adam_gate_load(gate, st, gt)) return;
    lamb_moments<T, T>(a, np, div, gt);
}

template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_master_moments_gated_kernel(LambArgs<float, kLambMasterSeg> a, Div np, int div,
                                     const kf_step_gate *__restrict__ gate,
                                     const kf_step_state *__restrict__ st)
{
    AdamGate<float> gt;
    if (adam_gate_load(gate, st, gt)) return;
    lamb_moments<float, T>(a, np, div, gt);
}

// ---- the trust ratios ----------------------------------------------------------

struct TrustArgs {
    double lr[kTrustGroups];
    int adapt[kTrustGroups];
    int g0, ng;  // this launch serves groups [g0, g0 + ng)
};

// One lane per tensor, fp64, one IEEE operation per parenthesis.
__global__ void __launch_bounds__(kLambBlock)
    lamb_trust_kernel(const double *__restrict__ sq, int world, int ntensor,
                      const int *__restrict__ group_of, TrustArgs a, double clip,
                      double *__restrict__ nlr, double *__restrict__ ratio)
{
    const size_t t = static_cast<size_t>(blockIdx.x) * kLambBlock + threadIdx.x;
    if (t >= static_cast<size_t>(ntensor)) return;
    const int j = group_of[t] - a.g0;
    if (j < 0 || j >= a.ng) return;
    const size_t row = 2 * static_cast<size_t>(ntensor);
    double P = 0.0, U = 0.0;
    for (int r = 0; r < world; ++r) {
        P = __dadd_rn(P, sq[r * row + t]);
        U = __dadd_rn(U, sq[r * row + ntensor + t]);
    }
    const double wn = __dsqrt_rn(P), un = __dsqrt_rn(U);
    // kTrustGroups selects instead of an indexed kernarg read (no scratch copy)
    double lr = 0.0;
    int adapt = 0;
#pragma unroll
    for (int i = 0; i < kTrustGroups; ++i) {
        if (i == j) {
            lr    = a.lr[i];
            adapt = a.adapt[i];
        }
    }
    double x = (adapt && wn > 0.0 && un > 0.0) ? __ddiv_rn(wn, un) : 1.0;
    if (clip > 0.0) x = x < clip ? x : clip;
    nlr[t]   = -__dmul_rn(lr, x);
    ratio[t] = x;
}

// Under a step gate: a skipped step leaves nlr[] and ratio[] as they were.
// lamb_trust_kernel's statements, written out again: `a` handed to a shared
// function is copied out of the kernarg segment first, and the parent's
// instruction stream would change with it.
__global__ void __launch_bounds__(kLambBlock)
    lamb_trust_gated_kernel(const double *__restrict__ sq, int world, int ntensor,
                            const int *__restrict__ group_of, TrustArgs a, double clip,
                            double *__restrict__ nlr, double *__restrict__ ratio,
                            const kf_step_gate *__restrict__ gate)
{
    if (gate->skip != 0) return;
    const size_t t = static_cast<size_t>(blockIdx.x) * kLambBlock + threadIdx.x;
    if (t >= static_cast<size_t>(ntensor)) return;
    const int j = group_of[t] - a.g0;
    if (j < 0 || j >= a.ng) return;
    const size_t row = 2 * static_cast<size_t>(ntensor);
    double P = 0.0, U = 0.0;
    for (int r = 0; r < world; ++r) {
        P = __dadd_rn(P, sq[r * row + t]);
        U = __dadd_rn(U, sq[r * row + ntensor + t]);
    }
    const double wn = __dsqrt_rn(P), un = __dsqrt_rn(U);
    // kTrustGroups selects instead of an indexed kernarg read (no scratch copy)
    double lr = 0.0;
    int adapt = 0;
#pragma unroll
    for (int i = 0; i < kTrustGroups; ++i) {
        if (i == j) {
            lr    = a.lr[i];
            adapt = a.adapt[i];
        }
    }
    double x = (adapt && wn > 0.0 && un > 0.0) ? __ddiv_rn(wn, un) : 1.0;
    if (clip > 0.0) x = x < clip ? x : clip;
    nlr[t]   = -__dmul_rn(lr, x);
    ratio[t] = x;
}

// ---- the apply pass --------------------------------------------------------------

// One row of the device table; row npiece is a sentinel whose blk0 is the grid.
struct LambPiece {
    void *p;        // parameters (or the fp32 master) of the piece
    const void *u;  // its update direction
    void *p16;      // master path: the 16-bit parameters, written only
    size_t n;
    unsigned head;  // elements before every array is 16-byte aligned (<= n)
    unsigned blk0;  // the piece's first block; it owns [blk0, next row's blk0)
    int tensor;
    int pad_;
};
static_assert(sizeof(LambPiece) == 48, "table row");

// The piece pointers come out of the table in memory (kf_segnorm.hip): cast to
// the global address space so that the loads and stores are global_*, not flat_*.
#define KF_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ u32x4 ldg4(const KF_GLOBAL char *base, size_t vi, bool nt)
{
    const KF_GLOBAL u32x4 *p = reinterpret_cast<const KF_GLOBAL u32x4 *>(base) + vi;
    return nt ? __builtin_nontemporal_load(p) : *p;
}
__device__ __forceinline__ void stg4(KF_GLOBAL char *base, size_t vi, const u32x4 &raw)
{
    KF_GLOBAL u32x4 *p = reinterpret_cast<KF_GLOBAL u32x4 *>(base) + vi;
    if constexpr (KF_LAMB_APPLY_ST_NT != 0) __builtin_nontemporal_store(raw, p);
    else *p = raw;
}

// C: float or double; T16: void (no 16-bit copy), bf16_t or f16_t.
template <typename C, typename T16>
__device__ __forceinline__ void apply_unit(KF_GLOBAL char *vp, KF_GLOBAL char *v16, size_t ui,
                                           const u32x4 &rp, const u32x4 &ru, C s)
{
    using SV        = SgdVec<C>;
    using X         = typename SV::X;
    constexpr int H = SV::N / 2;
    X p[H], u[H];
    SV::unpack(rp, p);
    SV::unpack(ru, u);
#pragma unroll
    for (int i = 0; i < H; ++i) p[i] = p[i] + s * u[i];
    stg4(vp, ui, SV::pack(p));
    if constexpr (!std::is_void<T16>::value) {
        u32x2 out;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            out[i] = static_cast<unsigned>(SgdElt<T16>::narrow(p[i].x)) |
                     (static_cast<unsigned>(SgdElt<T16>::narrow(p[i].y)) << 16);
        }
        *(reinterpret_cast<KF_GLOBAL u32x2 *>(v16) + ui) = out;
    }
}

// Block `blk` of the `nblk` of one piece. Elements [0, head) and
// [head + nunit * N, n) go one per lane of block 0 (fewer than 8 + N of them),
// the rest as 16-byte units from the piece's first aligned index.
template <typename C, typename T16>
__device__ __forceinline__ void apply_body(const LambPiece &d, size_t blk, size_t nblk, C s)
{
    constexpr int N = SgdVec<C>::N;
    constexpr int U = kApplyUnroll, B = kLambBlock;
    constexpr bool M = !std::is_void<T16>::value;
    KF_GLOBAL C *sp              = (KF_GLOBAL C *)d.p;
    const KF_GLOBAL C *su        = (const KF_GLOBAL C *)d.u;
    KF_GLOBAL uint16_t *s16      = (KF_GLOBAL uint16_t *)d.p16;
    const size_t n     = d.n;
    const size_t head  = d.head;
    const size_t nunit = (n - head) / N;
    const size_t vend  = head + nunit * N;
    const size_t nedge = head + (n - vend);

    if (blk == 0 && threadIdx.x < nedge) {
        const size_t t = threadIdx.x;
        const size_t i = t < head ? t : vend + (t - head);
        const C x      = sp[i] + s * su[i];
        sp[i]          = x;
        if constexpr (M) s16[i] = SgdElt<typename std::conditional<M, T16, float>::type>::narrow(x);
    }

    KF_GLOBAL char *vp        = reinterpret_cast<KF_GLOBAL char *>(sp + head);
    const KF_GLOBAL char *vu  = reinterpret_cast<const KF_GLOBAL char *>(su + head);
    KF_GLOBAL char *v16       = M ? reinterpret_cast<KF_GLOBAL char *>(s16 + head) : nullptr;
    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nunit + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u0 = t * tile + threadIdx.x;
        if (u0 + (U - 1) * B < nunit) {
            u32x4 rp[U], ru[U];
#pragma unroll
            for (int u = 0; u < U; ++u) ru[u] = ldg4(vu, u0 + u * B, true);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ldg4(vp, u0 + u * B, KF_LAMB_APPLY_P_NT != 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) apply_unit<C, T16>(vp, v16, u0 + u * B, rp[u], ru[u], s);
        } else {
            for (int u = 0; u < U; ++u) {
                const size_t ui = u0 + u * B;
                if (ui >= nunit) break;
                const u32x4 ru = ldg4(vu, ui, true), rp = ldg4(vp, ui, KF_LAMB_APPLY_P_NT != 0);
                apply_unit<C, T16>(vp, v16, ui, rp, ru, s);
            }
        }
    }
}

// Block b works for the last piece s whose blk0 <= b (kf_segnorm.hip's search:
// every piece of the table has at least one block).
template <typename C, typename T16>
__device__ __forceinline__ void lamb_apply(const LambPiece *__restrict__ tab, int npiece,
                                           const double *__restrict__ nlr)
{
    const unsigned b = blockIdx.x;
    int lo = 0, hi = npiece - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b >= tab[mid].blk0) lo = mid;
        else hi = mid - 1;
    }
    const LambPiece d   = tab[lo];
    const unsigned next = tab[lo + 1].blk0;
    const C s           = static_cast<C>(nlr[d.tensor]);
    apply_body<C, T16>(d, b - d.blk0, next - d.blk0, s);
}

template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_apply_kernel(const LambPiece *__restrict__ tab, int npiece, const double *__restrict__ nlr)
{
    lamb_apply<T, void>(tab, npiece, nlr);
}

template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_master_apply_kernel(const LambPiece *__restrict__ tab, int npiece,
                             const double *__restrict__ nlr)
{
    lamb_apply<float, T>(tab, npiece, nlr);
}

// Under a step gate: a skipped step returns before the table, p, u or p16 are
// loaded.
template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_apply_gated_kernel(const LambPiece *__restrict__ tab, int npiece,
                            const double *__restrict__ nlr, const kf_step_gate *__restrict__ gate)
{
    if (gate->skip != 0) return;
    lamb_apply<T, void>(tab, npiece, nlr);
}

template <typename T>
__global__ void __launch_bounds__(kLambBlock)
    lamb_master_apply_gated_kernel(const LambPiece *__restrict__ tab, int npiece,
                                   const double *__restrict__ nlr,
                                   const kf_step_gate *__restrict__ gate)
{
    if (gate->skip != 0) return;
    lamb_apply<float, T>(tab, npiece, nlr);
}

}  // namespace kf

struct kf_lamb_apply {
    kf::LambPiece *tab = nullptr;  // device, npiece + 1 rows (non-empty pieces only)
    int npiece         = 0;
    unsigned blocks    = 0;
    KungFu_Datatype dt = KungFu_FLOAT;
};

namespace
{
using namespace kf;

constexpr UpdateFail fail_moments{"kf_lamb_moments_batch"};
constexpr UpdateFail fail_master{"kf_lamb_master_moments_batch"};
constexpr UpdateFail fail_trust{"kf_lamb_trust_update"};
constexpr UpdateFail fail_create{"kf_lamb_apply_create"};
constexpr UpdateFail fail_run{"kf_lamb_apply_run"};
constexpr UpdateFail fail_moments_gated{"kf_lamb_moments_batch_gated"};
constexpr UpdateFail fail_master_gated{"kf_lamb_master_moments_batch_gated"};
constexpr UpdateFail fail_trust_gated{"kf_lamb_trust_update_gated"};
constexpr UpdateFail fail_run_gated{"kf_lamb_apply_run_gated"};

// C: compute type, NSEG: segments per launch. one: hyper[0] is every
// segment's (the gated entries), else hyper[b] is segment b's.
template <typename C, int NSEG, typename LAUNCH>
int launch_moments(const void *const *ps, const void *const *gs, void *const *ms, void *const *vs,
                   void *const *us, const size_t *counts, int nb, const kf_adam_hyper *hyper,
                   LAUNCH &&launch, bool one = false)
{
    return plan_update_batch<LambArgs<C, NSEG>>(
        counts, nb, SgdVec<C>::N, static_cast<size_t>(kLambBlock) * kLambUnroll,
        [&](LambSeg<C> &g, int b) {
            g.p = ps[b];
            g.g = gs[b];
            g.m = ms[b];
            g.v = vs[b];
            g.u = us[b];
            g.n = counts[b];
            lamb_scalars<C>(g.k, hyper[one ? 0 : b]);
        },
        launch);
}

// All four moments entries: every check comes before any HIP call, the dtype
// before the tables. bad_dtype: the refusal's text, or nullptr where dt is fine.
int moments_checks(const UpdateFail &fail, const void *const *ps, const void *const *gs,
                   void *const *ms, void *const *vs, void *const *us, const size_t *counts, int nb,
                   int np, const kf_adam_hyper *&hyper, UpdateGate *g, const char *bad_dtype)
{
    return check_update_batch(
        fail, {{ps, 16, kOff16}, {gs, 16, kOff16}, {ms, 16, kOff16}, {vs, 16, kOff16},
               {us, 16, kOff16}},
        {}, counts, nb, np, hyper, g, true,
        [&]() -> int { return bad_dtype ? fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", bad_dtype) : KF_OK; },
        no_check, no_check);
}

// gate == nullptr: the parent kernel
template <typename T>
void launch_apply(const kf_lamb_apply *p, const double *nlr, hipStream_t s,
                  const kf_step_gate *gate = nullptr)
{
    if (gate) {
        lamb_apply_gated_kernel<T><<<p->blocks, kLambBlock, 0, s>>>(p->tab, p->npiece, nlr, gate);
    } else {
        lamb_apply_kernel<T><<<p->blocks, kLambBlock, 0, s>>>(p->tab, p->npiece, nlr);
    }
}
template <typename T>
void launch_master_apply(const kf_lamb_apply *p, const double *nlr, hipStream_t s,
                         const kf_step_gate *gate = nullptr)
{
    if (gate) {
        lamb_master_apply_gated_kernel<T>
            <<<p->blocks, kLambBlock, 0, s>>>(p->tab, p->npiece, nlr, gate);
    } else {
        lamb_master_apply_kernel<T><<<p->blocks, kLambBlock, 0, s>>>(p->tab, p->npiece, nlr);
    }
}

// Both trust entries: every check comes before any HIP call. gate == nullptr:
// the parent kernel.
int trust_entry(const UpdateFail &fail, const double *sq, int world, int ntensor,
                const int *group_of, const kf_lamb_group *groups, int ngroup, double trust_clip,
                double *nlr, double *ratio, const kf_step_gate *gate, void *stream)
{
    if (world < 1 || ntensor < 1 || ngroup < 1) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "world, ntensor and ngroup must be at least 1");
    }
    if (!sq || !group_of || !groups || !nlr || !ratio) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    }
    if (trust_clip != trust_clip) return fail(KF_ERR_ARG, "KF_ERR_ARG", "trust_clip is NaN");
    hipStream_t s       = static_cast<hipStream_t>(stream);
    const unsigned grid = (static_cast<unsigned>(ntensor) + kLambBlock - 1) / kLambBlock;
    for (int g0 = 0; g0 < ngroup; g0 += kTrustGroups) {
        TrustArgs a;
        a.g0 = g0;
        a.ng = ngroup - g0 < kTrustGroups ? ngroup - g0 : kTrustGroups;
        for (int i = 0; i < kTrustGroups; ++i) {
            a.lr[i]    = i < a.ng ? groups[g0 + i].lr : 0.0;
            a.adapt[i] = i < a.ng ? (groups[g0 + i].adapt != 0) : 0;
        }
        if (gate) {
            lamb_trust_gated_kernel<<<grid, kLambBlock, 0, s>>>(sq, world, ntensor, group_of, a,
                                                                trust_clip, nlr, ratio, gate);
        } else {
            lamb_trust_kernel<<<grid, kLambBlock, 0, s>>>(sq, world, ntensor, group_of, a,
                                                          trust_clip, nlr, ratio);
        }
        const int rc = launch_status(fail);
        if (rc != KF_OK) return rc;
    }
    return KF_OK;
}

// Both apply entries.
int apply_entry(const UpdateFail &fail, kf_lamb_apply *p, const double *nlr,
                const kf_step_gate *gate, void *stream)
{
    if (p->blocks == 0) return KF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p->dt) {
    case KungFu_FLOAT: launch_apply<float>(p, nlr, s, gate); break;
    case KungFu_DOUBLE: launch_apply<double>(p, nlr, s, gate); break;
    case KungFu_BFLOAT16: launch_master_apply<bf16_t>(p, nlr, s, gate); break;
    default: launch_master_apply<f16_t>(p, nlr, s, gate); break;
    }
    return launch_status(fail);
}

}  // namespace

extern "C" {

int kf_lamb_moments_batch(const void *const *params, const void *const *grads,
                          void *const *exp_avgs, void *const *exp_avg_sqs, void *const *updates,
                          const size_t *counts, int nb, KungFu_Datatype dt, int np,
                          const kf_adam_hyper *hyper, void *stream)
{
    const UpdateFail &fail = fail_moments;
    const int rc = moments_checks(
        fail, params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, np, hyper, nullptr,
        dt == KungFu_FLOAT || dt == KungFu_DOUBLE ? nullptr
        : "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch)");
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    if (dt == KungFu_FLOAT) {
        return launch_moments<float, kLambSeg>(
            params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, hyper,
            [&](unsigned gx, unsigned gy, const LambArgs<float, kLambSeg> &a) {
                lamb_moments_kernel<float><<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div);
                return launch_status(fail);
            });
    }
    return launch_moments<double, kLambSeg>(
        params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, hyper,
        [&](unsigned gx, unsigned gy, const LambArgs<double, kLambSeg> &a) {
            lamb_moments_kernel<double><<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div);
            return launch_status(fail);
        });
}

int kf_lamb_master_moments_batch(const void *const *grads16, const void *const *masters,
                                 void *const *exp_avgs, void *const *exp_avg_sqs,
                                 void *const *updates, const size_t *counts, int nb,
                                 KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                 void *stream)
{
    const UpdateFail &fail = fail_master;
    const int rc = moments_checks(
        fail, masters, grads16, exp_avgs, exp_avg_sqs, updates, counts, nb, np, hyper, nullptr,
        dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16 ? nullptr
        : "bf16 and f16 gradients only (f32 and f64 take kf_lamb_moments_batch)");
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    auto launch   = [&](unsigned gx, unsigned gy, const LambArgs<float, kLambMasterSeg> &a) {
        if (dt == KungFu_BFLOAT16) {
            lamb_master_moments_kernel<bf16_t><<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div);
        } else {
            lamb_master_moments_kernel<f16_t><<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div);
        }
        return launch_status(fail);
    };
    return launch_moments<float, kLambMasterSeg>(masters, grads16, exp_avgs, exp_avg_sqs, updates,
                                                 counts, nb, hyper, launch);
}

int kf_lamb_trust_update(const double *sq, int world, int ntensor, const int *group_of,
                         const kf_lamb_group *groups, int ngroup, double trust_clip, double *nlr,
                         double *ratio, void *stream)
{
    return trust_entry(fail_trust, sq, world, ntensor, group_of, groups, ngroup, trust_clip, nlr,
                       ratio, nullptr, stream);
}

int kf_lamb_trust_update_gated(const double *sq, int world, int ntensor, const int *group_of,
                               const kf_lamb_group *groups, int ngroup, double trust_clip,
                               double *nlr, double *ratio, const kf_step_gate *gate, void *stream)
{
    if (!gate) return fail_trust_gated(KF_ERR_ARG, "KF_ERR_ARG", "null gate");
    return trust_entry(fail_trust_gated, sq, world, ntensor, group_of, groups, ngroup, trust_clip,
                       nlr, ratio, gate, stream);
}

int kf_lamb_moments_batch_gated(const void *const *params, const void *const *grads,
                                void *const *exp_avgs, void *const *exp_avg_sqs,
                                void *const *updates, const size_t *counts, int nb,
                                KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                const kf_step_gate *gate, const kf_step_state *state, void *stream)
{
    const UpdateFail &fail = fail_moments_gated;
    UpdateGate g = {gate, state, {}};
    const int rc = moments_checks(
        fail, params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, np, hyper, &g,
        dt == KungFu_FLOAT || dt == KungFu_DOUBLE ? nullptr
        : "f32 and f64 only (bf16 and f16 take kf_lamb_master_moments_batch_gated)");
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    if (dt == KungFu_FLOAT) {
        return launch_moments<float, kLambSeg>(
            params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, hyper,
            [&](unsigned gx, unsigned gy, const LambArgs<float, kLambSeg> &a) {
                lamb_moments_gated_kernel<float>
                    <<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div, gate, state);
                return launch_status(fail);
            },
            true);
    }
    return launch_moments<double, kLambSeg>(
        params, grads, exp_avgs, exp_avg_sqs, updates, counts, nb, hyper,
        [&](unsigned gx, unsigned gy, const LambArgs<double, kLambSeg> &a) {
            lamb_moments_gated_kernel<double>
                <<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div, gate, state);
            return launch_status(fail);
        },
        true);
}

int kf_lamb_master_moments_batch_gated(const void *const *grads16, const void *const *masters,
                                       void *const *exp_avgs, void *const *exp_avg_sqs,
                                       void *const *updates, const size_t *counts, int nb,
                                       KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                       const kf_step_gate *gate, const kf_step_state *state,
                                       void *stream)
{
    const UpdateFail &fail = fail_master_gated;
    UpdateGate g = {gate, state, {}};
    const int rc = moments_checks(
        fail, masters, grads16, exp_avgs, exp_avg_sqs, updates, counts, nb, np, hyper, &g,
        dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16 ? nullptr
        : "bf16 and f16 gradients only (f32 and f64 take kf_lamb_moments_batch_gated)");
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    auto launch   = [&](unsigned gx, unsigned gy, const LambArgs<float, kLambMasterSeg> &a) {
        if (dt == KungFu_BFLOAT16) {
            lamb_master_moments_gated_kernel<bf16_t>
                <<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div, gate, state);
        } else {
            lamb_master_moments_gated_kernel<f16_t>
                <<<dim3(gx, gy), kLambBlock, 0, s>>>(a, dv, div, gate, state);
        }
        return launch_status(fail);
    };
    return launch_moments<float, kLambMasterSeg>(masters, grads16, exp_avgs, exp_avg_sqs, updates,
                                                 counts, nb, hyper, launch, true);
}

kf_lamb_apply_t *kf_lamb_apply_create(void *const *params, const void *const *updates,
                                      void *const *params16, const size_t *counts,
                                      const int *tensors, int npiece, int ntensor,
                                      KungFu_Datatype dt)
{
    const UpdateFail &fail = fail_create;
    if (npiece < 0 || (npiece > 0 && (!params || !updates || !counts || !tensors))) {
        fail(KF_ERR_ARG, "KF_ERR_ARG", "null table, or npiece < 0");
        return nullptr;
    }
    const bool master = dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16;
    if (!master && dt != KungFu_FLOAT && dt != KungFu_DOUBLE) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "f32 and f64, or bf16 and f16 with master weights");
        return nullptr;
    }
    if (master && npiece > 0 && !params16) {
        fail(KF_ERR_ARG, "KF_ERR_ARG", "bf16 and f16 need the 16-bit parameter pointers");
        return nullptr;
    }
    const size_t sz   = dt == KungFu_DOUBLE ? 8 : 4;  // of params[] and updates[]
    const size_t unit = 16 / sz;                      // elements of a 16-byte unit
    const size_t per  = static_cast<size_t>(kLambBlock) * kApplyUnroll * kApplyTiles * unit;
    auto addr         = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    std::vector<LambPiece> rows;
    size_t blocks = 0;
    for (int i = 0; i < npiece; ++i) {
        const size_t n = counts[i];
        if (n == 0) continue;
        if (tensors[i] < 0 || tensors[i] >= ntensor) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "tensor index outside [0, ntensor)");
            return nullptr;
        }
        if (!params[i] || !updates[i] || (master && !params16[i])) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty piece");
            return nullptr;
        }
        if (addr(params[i]) % sz || addr(updates[i]) % sz || (master && addr(params16[i]) % 2)) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "pointer not aligned to the element");
            return nullptr;
        }
        // the first index at which every array of the piece is 16-byte aligned
        size_t head = 0;
        const size_t span = master ? 8 : unit;
        for (; head < span; ++head) {
            if ((addr(params[i]) + head * sz) % 16 == 0 && (addr(updates[i]) + head * sz) % 16 == 0 &&
                (!master || (addr(params16[i]) + head * 2) % 16 == 0)) {
                break;
            }
        }
        if (head == span) {
            fail(KF_ERR_ARG, "KF_ERR_ARG",
                 "a piece's arrays must share their element offset from a 16-byte boundary");
            return nullptr;
        }
        if (head > n) head = n;
        LambPiece r;
        r.p      = params[i];
        r.u      = updates[i];
        r.p16    = master ? params16[i] : nullptr;
        r.n      = n;
        r.head   = static_cast<unsigned>(head);
        r.blk0   = static_cast<unsigned>(blocks);
        r.tensor = tensors[i];
        r.pad_   = 0;
        rows.push_back(r);
        size_t nb = (n + per - 1) / per;  // kApplyTiles tiles per block, then they stride
        if (nb > 0x10000u) nb = 0x10000u;
        blocks += nb;
        if (blocks > 0x7fffffffu) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "more than 2^31 - 1 blocks");
            return nullptr;
        }
    }
    LambPiece end{};
    end.blk0 = static_cast<unsigned>(blocks);
    rows.push_back(end);
    kf_lamb_apply *p = new kf_lamb_apply;
    p->npiece        = static_cast<int>(rows.size()) - 1;
    p->blocks        = static_cast<unsigned>(blocks);
    p->dt            = dt;
    const size_t tb  = rows.size() * sizeof(LambPiece);
    hipError_t e     = hipMalloc(reinterpret_cast<void **>(&p->tab), tb);
    if (e == hipSuccess) e = hipMemcpy(p->tab, rows.data(), tb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fail(KF_ERR_HIP, "KF_ERR_HIP", hipGetErrorString(e));
        kf_lamb_apply_destroy(p);
        return nullptr;
    }
    return p;
}

int kf_lamb_apply_run(kf_lamb_apply_t *p, const double *nlr, void *stream)
{
    if (!p || !nlr) return fail_run(KF_ERR_ARG, "KF_ERR_ARG", "null plan or nlr");
    return apply_entry(fail_run, p, nlr, nullptr, stream);
}

int kf_lamb_apply_run_gated(kf_lamb_apply_t *p, const double *nlr, const kf_step_gate *gate,
                            void *stream)
{
    if (!p || !nlr) return fail_run_gated(KF_ERR_ARG, "KF_ERR_ARG", "null plan or nlr");
    if (!gate) return fail_run_gated(KF_ERR_ARG, "KF_ERR_ARG", "null gate");
    return apply_entry(fail_run_gated, p, nlr, gate, stream);
}

void kf_lamb_apply_destroy(kf_lamb_apply_t *p)
{
    if (!p) return;
    if (p->tab) (void)hipFree(p->tab);
    delete p;
}

}  // extern "C"
