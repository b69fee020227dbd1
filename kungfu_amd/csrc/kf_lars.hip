// kf_lars.hip — LARS on the sharded SGD step (include/kungfu_amd.h "LARS",
// DESIGN.md §23): a layer-wise trust ratio in front of torch.optim.SGD's
// arithmetic, where a tensor's elements are spread over the ranks' shards.
//
//   reduce-scatter(grads) -> segmented norms of the (p, g) pieces (kf_segnorm),
//                            all-gather of the sums
//                         -> trust: coef[t] = {ratio, wd, mu, c, nlr, flags}
//                         -> [own pieces: g/np, +wd*p, *ratio, momentum, p += nlr*g]
//                         -> all-gather(params)
//
// Two kernels:
//   * lars_trust_kernel: one lane per tensor, fp64. It folds the gathered sums
//     in rank order and writes the tensor's coefficient row to HBM, so the
//     apply pass takes every per-tensor scalar from device memory;
//   * lars_apply_kernel: one launch over all "tensor ∩ own shard" pieces
//     through a table in HBM (kf_lamb.hip's apply plan: a blk0 column with a
//     sentinel row, searched per block). Per piece it streams g, m and p in
//     and p, m and (master path) the 16-bit parameters out: 20 bytes per f32
//     element, 18 + 2 on the master path, where the gradient is 16 bits wide
//     beside fp32 master and momentum. A block reads its tensor's row once;
//     whether the momentum stream is read, written or left alone is decided
//     per block from the row's flags, the /np mode per launch.
//
// The arithmetic is kf_sgd.hip's (kf_sgd_elt.hpp), one IEEE operation per
// parenthesis, no contraction (the pragma of kf_reduce_kernels.hpp and
// -ffp-contract=off). No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_sgd_elt.hpp"
#include "kf_update_batch.hpp"

// 16-byte units per lane per tile, and the cache policy of the streams that
// are both read and written (1 = non-temporal); the measured ones (DESIGN.md
// §23). g is read once and always loaded non-temporally.
#ifndef KF_LARS_UNROLL
#define KF_LARS_UNROLL 4
#endif
#ifndef KF_LARS_LD_NT
#define KF_LARS_LD_NT 1
#endif
#ifndef KF_LARS_ST_NT
#define KF_LARS_ST_NT 0
#endif

namespace kf
{
constexpr int kLarsBlock  = 256;
constexpr int kLarsUnroll = KF_LARS_UNROLL;
constexpr int kLarsGroups = 16;  // param groups per trust launch
constexpr int kLarsCoef   = KF_LARS_COEF_DOUBLES;
constexpr int kLarsMomentum = 1, kLarsNesterov = 2, kLarsFirst = 4;  // a row's flags

// ---- the trust kernel ------------------------------------------------------------

struct LarsTrustArgs {
    double wd[kLarsGroups], mu[kLarsGroups], c[kLarsGroups], nlr[kLarsGroups];
    double tc[kLarsGroups], eps[kLarsGroups];
    int flags[kLarsGroups], adapt[kLarsGroups];
    int g0, ng;  // this launch serves groups [g0, g0 + ng)
};

// One lane per tensor, fp64, one IEEE operation per parenthesis.
__global__ void __launch_bounds__(kLarsBlock)
    lars_trust_kernel(const double *__restrict__ sq, int world, int ntensor,
                      const int *__restrict__ group_of, LarsTrustArgs a, int np,
                      double *__restrict__ coef, double *__restrict__ ratio)
{
    const size_t t = static_cast<size_t>(blockIdx.x) * kLarsBlock + threadIdx.x;
    if (t >= static_cast<size_t>(ntensor)) return;
    const int j = group_of[t] - a.g0;
    if (j < 0 || j >= a.ng) return;
    const size_t row = 2 * static_cast<size_t>(ntensor);
    double P = 0.0, G = 0.0;
    for (int r = 0; r < world; ++r) {
        P = __dadd_rn(P, sq[r * row + t]);
        G = __dadd_rn(G, sq[r * row + ntensor + t]);
    }
    const double wn = __dsqrt_rn(P);
    double gn       = __dsqrt_rn(G);
    if (np > 0) gn = __ddiv_rn(gn, static_cast<double>(np));
    // kLarsGroups selects instead of an indexed kernarg read (no scratch copy)
    double wd = 0.0, mu = 0.0, c = 0.0, nlr = 0.0, tc = 0.0, eps = 0.0;
    int flags = 0, adapt = 0;
#pragma unroll
    for (int i = 0; i < kLarsGroups; ++i) {
        if (i == j) {
            wd    = a.wd[i];
            mu    = a.mu[i];
            c     = a.c[i];
            nlr   = a.nlr[i];
            tc    = a.tc[i];
            eps   = a.eps[i];
            flags = a.flags[i];
            adapt = a.adapt[i];
        }
    }
    double x = 1.0;
    if (adapt && wn > 0.0 && gn > 0.0) {
        const double num = __dmul_rn(tc, wn);
        const double den = __dadd_rn(__dadd_rn(gn, __dmul_rn(wd, wn)), eps);
        x                = __ddiv_rn(num, den);
    }
    double *o = coef + static_cast<size_t>(kLarsCoef) * t;
    o[0]      = x;
    o[1]      = wd;
    o[2]      = mu;
    o[3]      = c;
    o[4]      = nlr;
    o[5]      = static_cast<double>(flags);
    ratio[t]  = x;
}

// ---- the apply kernel ------------------------------------------------------------

// One row of the device table; row npiece is a sentinel whose blk0 is the grid.
struct LarsPiece {
    void *p;        // parameters (or the fp32 master) of the piece
    const void *g;  // its reduced gradient: p's type, or 16 bits on the master path
    void *m;        // its momentum, p's type
    void *p16;      // master path: the 16-bit parameters, written only
    size_t n;
    unsigned head;  // elements before every array is 16-byte aligned (<= n)
    unsigned blk0;  // the piece's first block; it owns [blk0, next row's blk0)
    int tensor;
    int pad_[3];
};
static_assert(sizeof(LarsPiece) == 64, "table row");

// A tensor's row in the compute type, uniform over the block.
template <typename C> struct LarsRow {
    C ratio, wd, mu, c, nlr;
    bool decay, nesterov;
};

// The piece pointers come out of the table in memory: cast to the global
// address space so that the loads and stores are global_*, not flat_*.
#define KF_GLOBAL __attribute__((address_space(1)))
typedef unsigned int lars_u32x2 __attribute__((ext_vector_type(2)));

template <int NT, typename R>
__device__ __forceinline__ R lars_ld(const KF_GLOBAL char *base, size_t vi)
{
    const KF_GLOBAL R *p = reinterpret_cast<const KF_GLOBAL R *>(base) + vi;
    if constexpr (NT != 0) return __builtin_nontemporal_load(p);
    else return *p;
}
template <int NT, typename R>
__device__ __forceinline__ void lars_st(KF_GLOBAL char *base, size_t vi, const R &raw)
{
    KF_GLOBAL R *p = reinterpret_cast<KF_GLOBAL R *>(base) + vi;
    if constexpr (NT != 0) __builtin_nontemporal_store(raw, p);
    else *p = raw;
}

// The gradient stream of a unit (16 bytes of the compute type C): G == C reads
// 16 bytes, a 16-bit G reads 8 bytes and widens (exactly).
template <typename C, typename G> struct LarsGrad {  // G: bf16_t or f16_t, C: float
    using R = lars_u32x2;
    using X = f32x2;
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
    __device__ static C scalar(const KF_GLOBAL void *g, size_t i)
    {
        return SgdElt<G>::widen(reinterpret_cast<const KF_GLOBAL uint16_t *>(g)[i]);
    }
};
template <typename C> struct LarsGrad<C, C> {
    using R = u32x4;
    using X = typename SgdElt<C>::X;
    __device__ static void unpack(const R &r, X (&x)[SgdVec<C>::N / 2]) { SgdVec<C>::unpack(r, x); }
    __device__ static C scalar(const KF_GLOBAL void *g, size_t i)
    {
        return reinterpret_cast<const KF_GLOBAL C *>(g)[i];
    }
};

// MODE: 0 = no momentum (m neither read nor written), 1 = a first step (m
// written), 2 = m read and written.
//
// H values (V = C) or H lane pairs (V = SgdElt<C>::X): g holds the reduced
// gradient on entry; p and, with MODE != 0, m are updated.
template <typename C, int DIV, int MODE, int H, typename V>
__device__ __forceinline__ void lars_math(V (&p)[H], V (&g)[H], V (&m)[H], const LarsRow<C> &k,
                                          const Div &d)
{
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = SgdDiv<C, DIV>::run(g[i], d);
    if (k.decay) {
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const V t = k.wd * p[i];
            g[i]      = g[i] + t;
        }
    }
#pragma unroll
    for (int i = 0; i < H; ++i) g[i] = k.ratio * g[i];
    if constexpr (MODE == 1) {
#pragma unroll
        for (int i = 0; i < H; ++i) m[i] = g[i];
    }
    if constexpr (MODE == 2) {
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const V t = k.mu * m[i];
            const V s = k.c * g[i];
            m[i]      = t + s;
        }
    }
    if constexpr (MODE != 0) {
        if (k.nesterov) {
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const V t = k.mu * m[i];
                g[i]      = g[i] + t;
            }
        } else {
#pragma unroll
            for (int i = 0; i < H; ++i) g[i] = m[i];
        }
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const V t = k.nlr * g[i];
        p[i]      = p[i] + t;
    }
}

// one unit: p stored, m with MODE != 0, the 16-bit parameters on the master path
template <typename C, typename G, typename T16, int DIV, int MODE>
__device__ __forceinline__ void lars_unit(KF_GLOBAL char *vp, KF_GLOBAL char *vm,
                                          KF_GLOBAL char *v16, size_t ui,
                                          const typename LarsGrad<C, G>::R &rg, const u32x4 &rm,
                                          const u32x4 &rp, const LarsRow<C> &k, const Div &d)
{
    using SV        = SgdVec<C>;
    using X         = typename SV::X;
    constexpr int H = SV::N / 2;
    X p[H], g[H], m[H];
    LarsGrad<C, G>::unpack(rg, g);
    SV::unpack(rp, p);
    if constexpr (MODE == 2) SV::unpack(rm, m);
    lars_math<C, DIV, MODE, H, X>(p, g, m, k, d);
    lars_st<KF_LARS_ST_NT>(vp, ui, SV::pack(p));
    if constexpr (MODE != 0) lars_st<KF_LARS_ST_NT>(vm, ui, SV::pack(m));
    if constexpr (!std::is_void<T16>::value) {
        lars_u32x2 out;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            out[i] = static_cast<unsigned>(SgdElt<T16>::narrow(p[i].x)) |
                     (static_cast<unsigned>(SgdElt<T16>::narrow(p[i].y)) << 16);
        }
        lars_st<KF_LARS_ST_NT>(v16, ui, out);
    }
}

// Block `blk` of the `nblk` of one piece. Elements [0, head) and
// [head + nunit * N, n) go one per lane of block 0 (fewer than 8 + N of them),
// the rest as 16-byte units from the piece's first aligned index.
template <typename C, typename G, typename T16, int DIV, int MODE>
__device__ __forceinline__ void lars_body(const LarsPiece &d, size_t blk, size_t nblk,
                                          const LarsRow<C> &k, const Div &dv)
{
    using LG        = LarsGrad<C, G>;
    using GR        = typename LG::R;
    constexpr int N = SgdVec<C>::N;
    constexpr int U = kLarsUnroll, B = kLarsBlock;
    constexpr bool M = !std::is_void<T16>::value;
    using S16 = SgdElt<typename std::conditional<M, T16, float>::type>;
    KF_GLOBAL C *sp         = (KF_GLOBAL C *)d.p;
    KF_GLOBAL C *sm         = (KF_GLOBAL C *)d.m;
    const KF_GLOBAL void *sg = (const KF_GLOBAL void *)d.g;
    KF_GLOBAL uint16_t *s16 = (KF_GLOBAL uint16_t *)d.p16;
    const size_t n     = d.n;
    const size_t head  = d.head;
    const size_t nunit = (n - head) / N;
    const size_t vend  = head + nunit * N;
    const size_t nedge = head + (n - vend);

    if (blk == 0 && threadIdx.x < nedge) {
        const size_t t = threadIdx.x;
        const size_t i = t < head ? t : vend + (t - head);
        C p[1] = {sp[i]}, g[1] = {LG::scalar(sg, i)}, m[1] = {C(0)};
        if constexpr (MODE == 2) m[0] = sm[i];
        lars_math<C, DIV, MODE, 1, C>(p, g, m, k, dv);
        sp[i] = p[0];
        if constexpr (MODE != 0) sm[i] = m[0];
        if constexpr (M) s16[i] = S16::narrow(p[0]);
    }

    constexpr size_t gsz     = M ? 2 : sizeof(C);
    KF_GLOBAL char *vp       = reinterpret_cast<KF_GLOBAL char *>(sp + head);
    KF_GLOBAL char *vm       = reinterpret_cast<KF_GLOBAL char *>(sm + head);
    const KF_GLOBAL char *vg = reinterpret_cast<const KF_GLOBAL char *>(sg) + head * gsz;
    KF_GLOBAL char *v16      = M ? reinterpret_cast<KF_GLOBAL char *>(s16 + head) : nullptr;
    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nunit + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u0 = t * tile + threadIdx.x;
        if (u0 + (U - 1) * B < nunit) {
            // full tile: every load issued before the first use
            GR rg[U];
            u32x4 rm[U], rp[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = lars_ld<1, GR>(vg, u0 + u * B);
            if constexpr (MODE == 2) {
#pragma unroll
                for (int u = 0; u < U; ++u) rm[u] = lars_ld<KF_LARS_LD_NT, u32x4>(vm, u0 + u * B);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = lars_ld<KF_LARS_LD_NT, u32x4>(vp, u0 + u * B);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                lars_unit<C, G, T16, DIV, MODE>(vp, vm, v16, u0 + u * B, rg[u], rm[u], rp[u], k, dv);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t ui = u0 + u * B;
                if (ui >= nunit) break;
                const GR rg = lars_ld<1, GR>(vg, ui);
                u32x4 rm    = {0, 0, 0, 0};
                if constexpr (MODE == 2) rm = lars_ld<KF_LARS_LD_NT, u32x4>(vm, ui);
                const u32x4 rp = lars_ld<KF_LARS_LD_NT, u32x4>(vp, ui);
                lars_unit<C, G, T16, DIV, MODE>(vp, vm, v16, ui, rg, rm, rp, k, dv);
            }
        }
    }
}

// Block b works for the last piece s whose blk0 <= b (every piece of the table
// has at least one block); its tensor's row is read once, through uniform
// addresses.
template <typename C, typename G, typename T16, int DIV>
__device__ __forceinline__ void lars_apply(const LarsPiece *__restrict__ tab, int npiece,
                                           const double *__restrict__ coef, const Div &dv)
{
    const unsigned b = blockIdx.x;
    int lo = 0, hi = npiece - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b >= tab[mid].blk0) lo = mid;
        else hi = mid - 1;
    }
    const LarsPiece d   = tab[lo];
    const unsigned next = tab[lo + 1].blk0;
    const double *row   = coef + static_cast<size_t>(kLarsCoef) * d.tensor;
    LarsRow<C> k;
    k.ratio         = static_cast<C>(row[0]);
    k.wd            = static_cast<C>(row[1]);
    k.mu            = static_cast<C>(row[2]);
    k.c             = static_cast<C>(row[3]);
    k.nlr           = static_cast<C>(row[4]);
    const int flags = static_cast<int>(row[5]);
    k.decay         = k.wd != C(0);
    k.nesterov      = (flags & kLarsNesterov) != 0;
    const size_t blk = b - d.blk0, nblk = next - d.blk0;
    if (!(flags & kLarsMomentum)) lars_body<C, G, T16, DIV, 0>(d, blk, nblk, k, dv);
    else if (flags & kLarsFirst) lars_body<C, G, T16, DIV, 1>(d, blk, nblk, k, dv);
    else lars_body<C, G, T16, DIV, 2>(d, blk, nblk, k, dv);
}

// T: float or double, the parameters' own type
template <typename T, int DIV>
__global__ void __launch_bounds__(kLarsBlock)
    lars_apply_kernel(const LarsPiece *__restrict__ tab, int npiece,
                      const double *__restrict__ coef, Div np)
{
    lars_apply<T, T, void, DIV>(tab, npiece, coef, np);
}

// T: bf16_t or f16_t, the type of the gradients and of the 16-bit parameters;
// master and momentum are fp32
template <typename T, int DIV>
__global__ void __launch_bounds__(kLarsBlock)
    lars_master_apply_kernel(const LarsPiece *__restrict__ tab, int npiece,
                             const double *__restrict__ coef, Div np)
{
    lars_apply<float, T, T, DIV>(tab, npiece, coef, np);
}

}  // namespace kf

struct kf_lars_apply {
    kf::LarsPiece *tab = nullptr;  // device, npiece + 1 rows (non-empty pieces only)
    int npiece         = 0;
    unsigned blocks    = 0;
    KungFu_Datatype dt = KungFu_FLOAT;
};

namespace
{
using namespace kf;

constexpr UpdateFail fail_trust{"kf_lars_trust_update"};
constexpr UpdateFail fail_create{"kf_lars_apply_create"};
constexpr UpdateFail fail_run{"kf_lars_apply_run"};

template <int DIV>
void launch_apply(const kf_lars_apply *p, const double *coef, const Div &dv, hipStream_t s)
{
    const unsigned g = p->blocks;
    switch (p->dt) {
    case KungFu_FLOAT:
        lars_apply_kernel<float, DIV><<<g, kLarsBlock, 0, s>>>(p->tab, p->npiece, coef, dv);
        break;
    case KungFu_DOUBLE:
        lars_apply_kernel<double, DIV><<<g, kLarsBlock, 0, s>>>(p->tab, p->npiece, coef, dv);
        break;
    case KungFu_BFLOAT16:
        lars_master_apply_kernel<bf16_t, DIV><<<g, kLarsBlock, 0, s>>>(p->tab, p->npiece, coef, dv);
        break;
    default:
        lars_master_apply_kernel<f16_t, DIV><<<g, kLarsBlock, 0, s>>>(p->tab, p->npiece, coef, dv);
        break;
    }
}

}  // namespace

extern "C" {

int kf_lars_trust_update(const double *sq, int world, int ntensor, const int *group_of,
                         const kf_lars_group *groups, int ngroup, int np, double *coef,
                         double *ratio, void *stream)
{
    const UpdateFail &fail = fail_trust;
    if (world < 1 || ntensor < 1 || ngroup < 1) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "world, ntensor and ngroup must be at least 1");
    }
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    if (!sq || !group_of || !groups || !coef || !ratio) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    }
    hipStream_t s       = static_cast<hipStream_t>(stream);
    const unsigned grid = (static_cast<unsigned>(ntensor) + kLarsBlock - 1) / kLarsBlock;
    for (int g0 = 0; g0 < ngroup; g0 += kLarsGroups) {
        LarsTrustArgs a{};
        a.g0 = g0;
        a.ng = ngroup - g0 < kLarsGroups ? ngroup - g0 : kLarsGroups;
        for (int i = 0; i < a.ng; ++i) {
            const kf_lars_group &h = groups[g0 + i];
            a.wd[i]    = h.weight_decay;
            a.mu[i]    = h.momentum;
            a.c[i]     = 1.0 - h.dampening;
            a.nlr[i]   = -h.lr;
            a.tc[i]    = h.trust_coefficient;
            a.eps[i]   = h.eps;
            a.flags[i] = (h.momentum != 0 ? kLarsMomentum : 0) | (h.nesterov ? kLarsNesterov : 0) |
                         (h.first ? kLarsFirst : 0);
            a.adapt[i] = h.adapt != 0;
        }
        lars_trust_kernel<<<grid, kLarsBlock, 0, s>>>(sq, world, ntensor, group_of, a, np, coef,
                                                      ratio);
        const int rc = launch_status(fail);
        if (rc != KF_OK) return rc;
    }
    return KF_OK;
}

size_t kf_lars_apply_tile(KungFu_Datatype dt)
{
    return static_cast<size_t>(kLarsBlock) * kLarsUnroll * (dt == KungFu_DOUBLE ? 2 : 4);
}

kf_lars_apply_t *kf_lars_apply_create(void *const *params, const void *const *grads,
                                      void *const *moms, void *const *params16,
                                      const size_t *counts, const int *tensors, int npiece,
                                      int ntensor, KungFu_Datatype dt)
{
    const UpdateFail &fail = fail_create;
    if (npiece < 0 || (npiece > 0 && (!params || !grads || !moms || !counts || !tensors))) {
        fail(KF_ERR_ARG, "KF_ERR_ARG", "null table, or npiece < 0");
        return nullptr;
    }
    const bool master = dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16;
    if (!master && dt != KungFu_FLOAT && dt != KungFu_DOUBLE) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "f32 and f64, or bf16 and f16 with master weights");
        return nullptr;
    }
    if (!master && params16) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "f32 and f64 take no 16-bit parameter pointers");
        return nullptr;
    }
    if (master && npiece > 0 && !params16) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "bf16 and f16 need the 16-bit parameter pointers");
        return nullptr;
    }
    const size_t sz   = dt == KungFu_DOUBLE ? 8 : 4;  // of params[] and moms[]
    const size_t gsz  = master ? 2 : sz;              // of grads[]
    const size_t unit = 16 / sz;                      // elements of a 16-byte unit
    const size_t per  = static_cast<size_t>(kLarsBlock) * kLarsUnroll * unit;
    auto addr         = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    std::vector<LarsPiece> rows;
    size_t blocks = 0;
    for (int i = 0; i < npiece; ++i) {
        const size_t n = counts[i];
        if (n == 0) continue;
        if (tensors[i] < 0 || tensors[i] >= ntensor) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "tensor index outside [0, ntensor)");
            return nullptr;
        }
        if (!params[i] || !grads[i] || !moms[i] || (master && !params16[i])) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty piece");
            return nullptr;
        }
        if (addr(params[i]) % sz || addr(moms[i]) % sz || addr(grads[i]) % gsz ||
            (master && addr(params16[i]) % 2)) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "pointer not aligned to the element");
            return nullptr;
        }
        // the first index at which every array of the piece is 16-byte aligned
        size_t head = 0;
        const size_t span = master ? 8 : unit;
        for (; head < span; ++head) {
            if ((addr(params[i]) + head * sz) % 16 == 0 && (addr(moms[i]) + head * sz) % 16 == 0 &&
                (addr(grads[i]) + head * gsz) % 16 == 0 &&
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
        LarsPiece r{};
        r.p      = params[i];
        r.g      = grads[i];
        r.m      = moms[i];
        r.p16    = master ? params16[i] : nullptr;
        r.n      = n;
        r.head   = static_cast<unsigned>(head);
        r.blk0   = static_cast<unsigned>(blocks);
        r.tensor = tensors[i];
        rows.push_back(r);
        size_t nb = (n + per - 1) / per;  // one tile per block, then they stride
        if (nb > 0x10000u) nb = 0x10000u;
        blocks += nb;
        if (blocks > 0x7fffffffu) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "more than 2^31 - 1 blocks");
            return nullptr;
        }
    }
    LarsPiece end{};
    end.blk0 = static_cast<unsigned>(blocks);
    rows.push_back(end);
    kf_lars_apply *p = new kf_lars_apply;
    p->npiece        = static_cast<int>(rows.size()) - 1;
    p->blocks        = static_cast<unsigned>(blocks);
    p->dt            = dt;
    const size_t tb  = rows.size() * sizeof(LarsPiece);
    hipError_t e     = hipMalloc(reinterpret_cast<void **>(&p->tab), tb);
    if (e == hipSuccess) e = hipMemcpy(p->tab, rows.data(), tb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fail(KF_ERR_HIP, "KF_ERR_HIP", hipGetErrorString(e));
        kf_lars_apply_destroy(p);
        return nullptr;
    }
    return p;
}

int kf_lars_apply_run(kf_lars_apply_t *p, const double *coef, int np, void *stream)
{
    const UpdateFail &fail = fail_run;
    if (!p || !coef) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null plan or coef");
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    if (p->blocks == 0) return KF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Div dv  = update_div(np);
    switch (update_div_code(np, dv)) {
    case 0: launch_apply<0>(p, coef, dv, s); break;
    case 1: launch_apply<1>(p, coef, dv, s); break;
    default: launch_apply<2>(p, coef, dv, s); break;
    }
    return launch_status(fail);
}

void kf_lars_apply_destroy(kf_lars_apply_t *p)
{
    if (!p) return;
    if (p->tab) (void)hipFree(p->tab);
    delete p;
}

}  // extern "C"
