// kf_lion.hip — Lion (Chen et al. 2023, "Symbolic Discovery of Optimization
// Algorithms") on the shard step, dense and over a 2-bit sign wire
// (include/kungfu_amd.h "Lion"):
//
//   dense:  reduce-scatter(grads) -> [own shard: lion_update_kernel]
//                                 -> all-gather(params)
//   signs:  reduce-scatter(grads) -> [own shard: lion_signs_kernel -> codes]
//                                 -> all-gather(codes, 2 bits per element)
//                                 -> [whole buckets: lion_apply_signs_kernel]
//
// Arithmetic, per element, f32, every parenthesis one IEEE operation (the
// __f*_rn intrinsics: nothing is contracted):
//
//   g  = np > 0 ? sum / np : sum
//   c  = (b1*m) + (c1*g)            m' = (b2*m) + (c2*g)
//   code = c > 0 ? 1 : c < 0 ? 3 : c == c ? 0 : 2
//   if decay: p = dk*p
//   code 1: p = p + nlr   code 3: p = p - nlr   code 2: p = quiet NaN
//   code 0: p stays (its very bits when there is no decay)
//
// bf16 widens g, m and p exactly, stores m' round-to-nearest-even and p with
// kf_adam_sr.hip's stochastic narrowing; the 16 random bits of element e of a
// bucket are the high half of one word of philox2x32_10(e >> 1, stream, key),
// so the dense kernel on a shard and the apply kernel on the same elements of
// a replica round alike, on every rank. p = apply(p, code) is ONE device
// function, which the dense kernel calls too: the two paths cannot differ.
//
// Two shapes.
//
// lion_update_kernel is kf_sgd.hip's: 256 lanes, a tile of U x 256 16-byte
// vectors per stream, vector-interleaved (lane l takes vectors l, l + 256, ..),
// the loads of g, p and m (12 for f32, 6 for bf16) issued before the
// arithmetic. Reads g, m, p; writes m, p: 5 accesses per element.
//
// lion_signs_kernel and lion_apply_signs_kernel are unit-major: a lane owns
// one unit of 16 consecutive elements (four 16-byte vectors per stream for
// f32, two for bf16), because the unit's 16 codes are ONE dword: they are
// or-ed together in one VGPR with shifts and leave (signs) or arrive (apply)
// as one 4-byte access per lane, 256 contiguous bytes per wave. No LDS, no
// atomics, no access narrower than a dword. signs reads g, m and writes m and
// 0.25 bytes of codes per element, never p; apply reads the code dword first,
// then p, and writes p.
//
// Counts are multiples of 32 elements (the MXFP8 wire's rule, which the
// optimizers' shards keep), so a segment is whole units and whole vectors:
// there is no scalar tail and no head. A piece's codes are n / 16 dwords
// padded with zero dwords to the next 16 bytes; the lanes whose unit index
// falls into the padding store the zeros.
//
// Tile depth and load / store policy: NOT measured for these kernels. The
// depth is kf_sgd.hip's register footprint (four vectors per lane and stream
// for f32; bf16 takes two, the same 4096 elements per tile), and the policy is
// the one kf_sgd.hip's A/B chose for the same streams: g (dead afterwards)
// and the codes (read once) non-temporal, p and m plain, stores plain.
// tools/bench_lion.py times the three kernels beside kf_sgd_update_batch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_philox.hpp"
#include "kf_sgd_elt.hpp"
#include "kf_update_batch.hpp"

#ifndef KF_LION_G_NT
#define KF_LION_G_NT 1
#endif
#ifndef KF_LION_PM_NT
#define KF_LION_PM_NT 0
#endif
#ifndef KF_LION_ST_NT
#define KF_LION_ST_NT 0
#endif
#ifndef KF_LION_CODE_NT
#define KF_LION_CODE_NT 1
#endif

namespace kf
{
constexpr int kLionSeg   = 32;
constexpr int kLionBlock = 256;
constexpr int kLionUnit  = 16;  // elements a lane owns in the signs and apply kernels: one code dword
constexpr int kLionTile  = 4096;  // elements of a tile, all three kernels, both dtypes

// One segment, every kernel's: the pointers it does not use are null.
struct LionSeg {
    void *p;
    const void *g;
    void *m;
    void *codes;  // signs writes them, apply reads them
    size_t n;
    uint64_t base;  // bf16: element index of the segment's first element in its bucket
    float b1, c1, b2, c2, dk, nlr;
    int decay;        // weight_decay != 0
    uint32_t stream;  // bf16: Philox counter word c1
};
struct LionArgs {
    LionSeg seg[kLionSeg];
    unsigned blk0[kLionSeg + 1];  // the search table (1-D grids only)
    int nseg;
};
static_assert(sizeof(LionSeg) == 80, "kernarg entry");
static_assert(sizeof(LionArgs) + sizeof(Div) + 2 * sizeof(uint32_t) <= 3072, "kernarg budget");

template <typename T> struct LionElt;
template <> struct LionElt<float> {
    static constexpr int N = 4;  // elements of a 16-byte vector
    static constexpr uint32_t kNaN = 0x7fc00000u;
};
template <> struct LionElt<bf16_t> {
    static constexpr int N = 8;
    static constexpr uint32_t kNaN = 0x7fc0u;
};

// V 16-byte vectors <-> V * N floats, in element order
template <typename T, int V>
__device__ __forceinline__ void lion_widen(const u32x4 (&r)[V], float (&x)[V * LionElt<T>::N])
{
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if constexpr (std::is_same<T, float>::value) {
                x[4 * v + w] = __uint_as_float(r[v][w]);
            } else {
                x[8 * v + 2 * w]     = __uint_as_float(r[v][w] << 16);
                x[8 * v + 2 * w + 1] = __uint_as_float(r[v][w] & 0xffff0000u);
            }
        }
    }
}

__device__ __forceinline__ float lion_div(float g, const Div &d, int div)
{
    return div == 0 ? g : (div == 1 ? __fmul_rn(g, d.fi) : __fdiv_rn(g, d.f));
}

// c's code and the new momentum of one element
__device__ __forceinline__ uint32_t lion_code(float g, float &m, const LionSeg &h)
{
    const float c  = __fadd_rn(__fmul_rn(h.b1, m), __fmul_rn(h.c1, g));
    m              = __fadd_rn(__fmul_rn(h.b2, m), __fmul_rn(h.c2, g));
    const uint32_t nz = (c > 0.0f) ? 1u : ((c < 0.0f) ? 3u : 0u);
    return (c == c) ? nz : 2u;
}

// The parameter after code k, as f32: codes 0 and 2 are the caller's (they
// are choices of bits, not arithmetic). p - nlr is p + (-nlr): the same IEEE
// operation, with the code's high bit as nlr's sign flip.
__device__ __forceinline__ float lion_step(float p, uint32_t k, const LionSeg &h)
{
    const float x = h.decay ? __fmul_rn(h.dk, p) : p;
    const float d = __uint_as_float(__float_as_uint(h.nlr) ^ ((k & 2u) << 30));
    return (k & 1u) ? __fadd_rn(x, d) : x;
}

// sr(x, r), r < 2^16, as 16 bits: kf_adam_sr.hip's narrowing (its sr_pair is
// that file's own; this is the same rule on one value).
__device__ __forceinline__ uint32_t lion_sr(float x, uint32_t r)
{
    const uint32_t s = (__float_as_uint(x) + r) >> 16;
    return __builtin_isfinite(x) ? s : static_cast<uint32_t>(f32_to_bf16(x));
}

// Apply the codes of V vectors (word: 2 bits per element, element i of the V
// vectors at bits 2i; V * N <= 16) to the raw parameter vectors r, in place.
// pair0: bf16, the Philox counter c0 of the first element pair.
template <typename T, int V>
__device__ __forceinline__ void lion_apply_vecs(u32x4 (&r)[V], uint32_t word, const LionSeg &h,
                                                uint32_t pair0, uint32_t key)
{
    constexpr int N = LionElt<T>::N;
    float x[V * N];
    lion_widen<T, V>(r, x);
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int i = 0; i < V * N; ++i) {
            const uint32_t k = (word >> (2 * i)) & 3u;
            const float y    = lion_step(x[i], k, h);
            // code 0 without decay: y is x, moved and not computed on, so its bits stay
            r[i / 4][i % 4] = k == 2u ? LionElt<float>::kNaN : __float_as_uint(y);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V * N / 2; ++j) {
            const Philox2 q   = philox2x32_10(pair0 + j, h.stream, key);
            const uint32_t old = r[j / 4][j % 4];
            uint32_t out       = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i       = 2 * j + e;
                const uint32_t k  = (word >> (2 * i)) & 3u;
                const uint32_t o  = (old >> (16 * e)) & 0xffffu;
                const uint32_t rp = (e ? q.b : q.a) >> 16;
                uint32_t s        = lion_sr(lion_step(x[i], k, h), rp);
                if (k == 0u && !h.decay) s = o;  // the very bits, a signalling NaN's too
                if (k == 2u) s = LionElt<bf16_t>::kNaN;
                out |= s << (16 * e);
            }
            r[j / 4][j % 4] = out;
        }
    }
}

// The codes of V vectors of g and m (m updated in place, as floats), element
// i's at bits 2i.
template <typename T, int V>
__device__ __forceinline__ uint32_t lion_code_vecs(const u32x4 (&rg)[V], u32x4 (&rm)[V],
                                                   const LionSeg &h, const Div &d, int div)
{
    constexpr int N = LionElt<T>::N;
    float g[V * N], m[V * N];
    lion_widen<T, V>(rg, g);
    lion_widen<T, V>(rm, m);
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < V * N; ++i) {
        word |= lion_code(lion_div(g[i], d, div), m[i], h) << (2 * i);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if constexpr (std::is_same<T, float>::value) {
                rm[v][w] = __float_as_uint(m[4 * v + w]);
            } else {
                rm[v][w] = static_cast<uint32_t>(f32_to_bf16(m[8 * v + 2 * w])) |
                           (static_cast<uint32_t>(f32_to_bf16(m[8 * v + 2 * w + 1])) << 16);
            }
        }
    }
    return word;
}

// ---- dense: kf_sgd.hip's tile ------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kLionBlock)
    lion_update_kernel(LionArgs a, Div np, int div, uint32_t key)
{
    constexpr int N = LionElt<T>::N, B = kLionBlock;
    constexpr int U = kLionTile / (B * N);  // 16-byte vectors per lane per stream per tile
    size_t blk, nblk;
    const LionSeg &h  = a.seg[batch_segment(a, blk, nblk)];
    const size_t nvec = h.n / N;
    const size_t tile = static_cast<size_t>(B) * U;
    const size_t ntiles = (nvec + tile - 1) / tile;
    const uint32_t pair0 = static_cast<uint32_t>(h.base >> 1);
    auto one = [&](size_t vi, const u32x4 &g, const u32x4 &p, const u32x4 &m) {
        const u32x4 rg[1] = {g};
        u32x4 rp[1] = {p}, rm[1] = {m};
        const uint32_t word = lion_code_vecs<T, 1>(rg, rm, h, np, div);
        lion_apply_vecs<T, 1>(rp, word, h, pair0 + static_cast<uint32_t>(vi) * (N / 2), key);
        st_u4<KF_LION_ST_NT>(h.p, vi, rp[0]);
        st_u4<KF_LION_ST_NT>(h.m, vi, rm[0]);
    };
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        if (v0 + (U - 1) * B < nvec) {
            // full tile: every load issued before the first use
            u32x4 rg[U], rp[U], rm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = ld_u4<KF_LION_G_NT>(h.g, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ld_u4<KF_LION_PM_NT>(h.p, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rm[u] = ld_u4<KF_LION_PM_NT>(h.m, v0 + u * B);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) one(v0 + u * B, rg[u], rp[u], rm[u]);
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t vi = v0 + u * B;
                if (vi >= nvec) break;
                one(vi, ld_u4<KF_LION_G_NT>(h.g, vi), ld_u4<KF_LION_PM_NT>(h.p, vi),
                    ld_u4<KF_LION_PM_NT>(h.m, vi));
            }
        }
    }
}

// ---- the sign wire: a lane owns 16 consecutive elements -----------------------
template <typename T>
__global__ void __launch_bounds__(kLionBlock)
    lion_signs_kernel(LionArgs a, Div np, int div)
{
    constexpr int V = kLionUnit / LionElt<T>::N;  // vectors of a unit: 4 (f32), 2 (bf16)
    size_t blk, nblk;
    const LionSeg &h    = a.seg[batch_segment(a, blk, nblk)];
    const size_t nunit  = h.n / kLionUnit;
    const size_t ndword = (nunit + 3) & ~static_cast<size_t>(3);  // with the padding to 16 bytes
    const size_t ntiles = (nunit + kLionBlock - 1) / kLionBlock;   // the padding never opens a tile
    uint32_t *codes     = static_cast<uint32_t *>(h.codes);
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u = t * kLionBlock + threadIdx.x;
        if (u < nunit) {
            u32x4 rg[V], rm[V];
#pragma unroll
            for (int v = 0; v < V; ++v) rg[v] = ld_u4<KF_LION_G_NT>(h.g, u * V + v);
#pragma unroll
            for (int v = 0; v < V; ++v) rm[v] = ld_u4<KF_LION_PM_NT>(h.m, u * V + v);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t word = lion_code_vecs<T, V>(rg, rm, h, np, div);
#pragma unroll
            for (int v = 0; v < V; ++v) st_u4<KF_LION_ST_NT>(h.m, u * V + v, rm[v]);
            codes[u] = word;
        } else if (u < ndword) {
            codes[u] = 0;  // the piece's padding, by the lanes that own it
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kLionBlock)
    lion_apply_signs_kernel(LionArgs a, uint32_t key)
{
    constexpr int V = kLionUnit / LionElt<T>::N;
    size_t blk, nblk;
    const LionSeg &h    = a.seg[batch_segment(a, blk, nblk)];
    const size_t nunit  = h.n / kLionUnit;
    const size_t ntiles = (nunit + kLionBlock - 1) / kLionBlock;
    const uint32_t *codes = static_cast<const uint32_t *>(h.codes);
    const uint32_t pair0  = static_cast<uint32_t>(h.base >> 1);
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u = t * kLionBlock + threadIdx.x;
        if (u >= nunit) break;
        // the code dword first, then the parameters it steers
        uint32_t word;
        if constexpr (KF_LION_CODE_NT) word = __builtin_nontemporal_load(codes + u);
        else word = codes[u];
        u32x4 rp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) rp[v] = ld_u4<KF_LION_PM_NT>(h.p, u * V + v);
        __builtin_amdgcn_sched_barrier(0);
        lion_apply_vecs<T, V>(rp, word, h, pair0 + static_cast<uint32_t>(u) * (kLionUnit / 2), key);
#pragma unroll
        for (int v = 0; v < V; ++v) st_u4<KF_LION_ST_NT>(h.p, u * V + v, rp[v]);
    }
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail_update{"kf_lion_update_batch"};
constexpr UpdateFail fail_signs{"kf_lion_signs_batch"};
constexpr UpdateFail fail_apply{"kf_lion_apply_signs_batch"};

constexpr uint64_t kMaxElement = 1ull << 33;  // a pair index is 32 bits

// The checks of the three entries, all before any HIP call, in one order: nb,
// the tables, the dtype, bf16's bases and streams, np, then per non-empty
// segment null pointers, alignment, count % 32, and for bf16 the base rules
// of kf_adam_sr_update_batch. np < 0 stands for "this entry has no np";
// sr: this entry draws random bits for bf16.
template <size_t K>
int lion_check(const UpdateFail &fail, const void *const *const (&tabs)[K], const size_t *counts,
               int nb, KungFu_Datatype dt, bool has_np, int np, const kf_lion_hyper *hyper, bool sr,
               const uint64_t *bases, const uint32_t *streams)
{
    if (nb < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "nb < 0");
    if (nb == 0) return KF_OK;
    bool null = !counts || !hyper;
    for (const void *const *t : tabs) null = null || !t;
    if (null) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    if (dt != KungFu_FLOAT && dt != KungFu_BFLOAT16) {
        // f16: there is no stochastic narrowing to f16 here, and rounded to
        // nearest a step of lr = 1e-4 is below half an ulp of every |p| >= 0.25
        // and would be dropped; f64 has no momentum worth saving on.
        return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE",
                    "f32 and bf16 only (f16 has no stochastic narrowing: round-to-nearest drops "
                    "updates below half an ulp)");
    }
    sr = sr && dt == KungFu_BFLOAT16;
    if (sr && (!bases || !streams)) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    if (has_np && np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] == 0) continue;
        bool none = false, off = false;
        for (const void *const *t : tabs) {
            none = none || !t[b];
            off  = off || off16(t[b]);
        }
        if (none) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty segment");
        if (off) return fail(KF_ERR_ARG, "KF_ERR_ARG", kOff16);
        if (counts[b] % 32) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "counts must be multiples of 32 elements");
        }
        if (!sr) continue;
        if (bases[b] % 8 != 0) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "bases must be multiples of 8 elements");
        }
        if (bases[b] > kMaxElement || counts[b] > kMaxElement - bases[b]) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "base + count must be at most 2^33");
        }
    }
    return KF_OK;
}

// c1, c2, dk and nlr in double, cast once
void lion_scalars(LionSeg &g, const kf_lion_hyper &h)
{
    g.b1    = static_cast<float>(h.beta1);
    g.c1    = static_cast<float>(1.0 - h.beta1);
    g.b2    = static_cast<float>(h.beta2);
    g.c2    = static_cast<float>(1.0 - h.beta2);
    g.dk    = static_cast<float>(1.0 - h.lr * h.weight_decay);
    g.nlr   = static_cast<float>(-h.lr);
    g.decay = h.weight_decay != 0 ? 1 : 0;
}

enum LionKernel { LION_UPDATE, LION_SIGNS, LION_APPLY };

template <typename T, LionKernel K>
int launch_lion(const UpdateFail &fail, void *const *params, const void *const *grads,
                void *const *moms, void *const *codes, const size_t *counts,
                const uint64_t *bases, const uint32_t *streams, int nb, int np,
                const kf_lion_hyper *hyper, uint32_t key, hipStream_t s)
{
    const Div dv     = update_div(np);
    const int div    = update_div_code(np, dv);
    const bool sr    = std::is_same<T, bf16_t>::value && K != LION_SIGNS;
    // a unit is what a lane loads at once: a vector (dense) or 16 elements
    const size_t elts = K == LION_UPDATE ? LionElt<T>::N : kLionUnit;
    return plan_update_batch<LionArgs>(
        counts, nb, elts, kLionTile / elts,
        [&](LionSeg &g, int b) {
            g.p      = params ? params[b] : nullptr;
            g.g      = grads ? grads[b] : nullptr;
            g.m      = moms ? moms[b] : nullptr;
            g.codes  = codes ? codes[b] : nullptr;
            g.n      = counts[b];
            g.base   = sr ? bases[b] : 0;
            g.stream = sr ? streams[b] : 0;
            lion_scalars(g, hyper[b]);
        },
        [&](unsigned gx, unsigned gy, const LionArgs &a) {
            if constexpr (K == LION_UPDATE) {
                lion_update_kernel<T><<<dim3(gx, gy), kLionBlock, 0, s>>>(a, dv, div, key);
            } else if constexpr (K == LION_SIGNS) {
                lion_signs_kernel<T><<<dim3(gx, gy), kLionBlock, 0, s>>>(a, dv, div);
            } else {
                lion_apply_signs_kernel<T><<<dim3(gx, gy), kLionBlock, 0, s>>>(a, key);
            }
            return launch_status(fail);
        });
}

}  // namespace

extern "C" {

size_t kf_lion_sign_bytes(size_t q) { return (q / 16 * 4 + 15) / 16 * 16; }

int kf_lion_update_batch(void *const *params, const void *const *grads, void *const *moms,
                         const size_t *counts, const uint64_t *bases, const uint32_t *streams,
                         int nb, KungFu_Datatype dt, int np, const kf_lion_hyper *hyper,
                         uint32_t key, void *stream)
{
    const void *const *const tabs[3] = {params, grads, moms};
    const int rc = lion_check(fail_update, tabs, counts, nb, dt, true, np, hyper, true, bases, streams);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) {
        return launch_lion<float, LION_UPDATE>(fail_update, params, grads, moms, nullptr, counts,
                                               bases, streams, nb, np, hyper, key, s);
    }
    return launch_lion<bf16_t, LION_UPDATE>(fail_update, params, grads, moms, nullptr, counts, bases,
                                            streams, nb, np, hyper, key, s);
}

int kf_lion_signs_batch(const void *const *grads, void *const *moms, void *const *codes,
                        const size_t *counts, int nb, KungFu_Datatype dt, int np,
                        const kf_lion_hyper *hyper, void *stream)
{
    const void *const *const tabs[3] = {grads, moms, codes};
    const int rc = lion_check(fail_signs, tabs, counts, nb, dt, true, np, hyper, false, nullptr, nullptr);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) {
        return launch_lion<float, LION_SIGNS>(fail_signs, nullptr, grads, moms, codes, counts,
                                              nullptr, nullptr, nb, np, hyper, 0, s);
    }
    return launch_lion<bf16_t, LION_SIGNS>(fail_signs, nullptr, grads, moms, codes, counts, nullptr,
                                           nullptr, nb, np, hyper, 0, s);
}

int kf_lion_apply_signs_batch(void *const *params, const void *const *codes, const size_t *counts,
                              const uint64_t *bases, const uint32_t *streams, int nb,
                              KungFu_Datatype dt, const kf_lion_hyper *hyper, uint32_t key,
                              void *stream)
{
    const void *const *const tabs[2] = {params, codes};
    const int rc = lion_check(fail_apply, tabs, counts, nb, dt, false, 0, hyper, true, bases, streams);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *const *cd = const_cast<void *const *>(reinterpret_cast<const void *const *>(codes));
    if (dt == KungFu_FLOAT) {
        return launch_lion<float, LION_APPLY>(fail_apply, params, nullptr, nullptr, cd, counts, bases,
                                              streams, nb, 0, hyper, key, s);
    }
    return launch_lion<bf16_t, LION_APPLY>(fail_apply, params, nullptr, nullptr, cd, counts, bases,
                                           streams, nb, 0, hyper, key, s);
}

}  // extern "C"
