// kf_adam8.hip — the Adam / AdamW update of a shard whose exp_avg and
// exp_avg_sq are held as block-wise 8-bit codes (include/kungfu_amd.h "8-bit
// block-wise state"; Dettmers et al., "8-bit Optimizers via
// Block-wise Quantization"):
//
//   reduce-scatter(grads) -> [own shard: dequantize m, v; kf_adam.hip's f32
//                             update; quantize m, v] -> all-gather(params)
//
// A block is 64 consecutive elements of a segment: 64 codes and one f32 scale
// per state. A segment reads g, p (4 B each), two codes and 2 x 4/64 B of
// scales and writes p, two codes and the scales: 16.25 bytes per element where
// kf_adam.hip moves 28. With a master copy (bf16 / f16 parameters) g and p16
// are 2 B each and the fp32 master takes p's place: also 16.25.
//
// Shape: kf_adam.hip's batched launch (kf_update_batch.hpp's planner and
// segment lookup), 256 lanes, a lane owns 4 consecutive elements per unit: one
// 16-byte access on the fp32 streams, one dword of codes per state. A block is
// then 16 consecutive lanes, one DPP row: the magnitude / sign reduction is
// four v_max_u32 with row_ror, after which every lane of the row holds the
// block's result. No LDS traffic and no barrier for the reduction. Both tables
// and their midpoints (4 KiB) are copied to LDS once per workgroup.
//
// The reduction's key. For one element, key = (bits(x) << 1) | (x >= 0): the
// magnitude's bits above a flag that says "not negative". The unsigned maximum
// of the keys is the largest magnitude, and of two elements of that magnitude
// the positive one; a NaN's magnitude bits exceed every number's, so a NaN
// wins the maximum and is seen in the result (mag > 0x7F800000). The maximum
// is an integer one on purpose: v_max_f32 returns the other operand for a NaN.
//
// The code of y is the number of midpoints below y. The 255 midpoints are held
// in LDS as an implicit search tree in breadth-first order (node i's children
// are 2i and 2i + 1): eight steps i = 2i + (E[i] < y) from i = 1 end at
// i = 256 + code. A level's nodes are consecutive words, so the first seven
// steps read at most one word per bank. A NaN y compares false eight times:
// code 0. A y on a midpoint takes the lower code.
//
// Arithmetic: m = T_s[code] * scale and v = T_u[code] * scale (one multiply
// each), adam_math<float, ...> of kf_adam_math.hpp on them, p from the
// unquantized results, then y = x / a with __fdiv_rn. No contraction.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_adam_math.hpp"
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal: kf_adam.hip's.
#ifndef KF_ADAM8_G_NT
#define KF_ADAM8_G_NT 1
#endif

namespace kf
{
constexpr int kAdam8Seg   = 24;
constexpr int kAdam8Block = 256;
constexpr int kAdam8Elts  = 4;   // elements per unit (one lane, one access)
constexpr int kAdam8Blk   = 64;  // elements per quantization block: 16 lanes
#ifndef KF_ADAM8_UNROLL
#define KF_ADAM8_UNROLL 1  // units per lane per tile: DESIGN.md §20 has 1, 2 and 4 measured
#endif
constexpr int kAdam8Unroll = KF_ADAM8_UNROLL;
static_assert(kAdam8Blk == 16 * kAdam8Elts, "a block is one DPP row");

// ---- the tables ---------------------------------------------------------------
// T[0]: signed (exp_avg), T[1]: unsigned (exp_avg_sq), ascending. E[w][i],
// i = 1..255: T[w]'s midpoints in breadth-first order of the search tree.
struct Adam8Tables {
    float T[2][256];
    float E[2][256];
};

constexpr double kAdam8Decade[7] = {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0};

// value k of decade i with n intervals, in double: one IEEE operation per
// parenthesis, as tests/adam8_ref.py writes it
constexpr double adam8_value(int i, int k, int n)
{
    const double b0 = 0.1 + ((0.9 * k) / n);
    const double b1 = 0.1 + ((0.9 * (k + 1)) / n);
    return (kAdam8Decade[i] * (b0 + b1)) / 2;
}

constexpr Adam8Tables make_adam8_tables()
{
    Adam8Tables t{};
    int at = 128;  // signed: 127 negatives, 0, 127 positives, 1
    t.T[0][127] = 0.0f;
    for (int i = 0; i < 7; ++i) {
        const int n = 1 << i;
        for (int k = 0; k < n; ++k, ++at) {
            const float x    = static_cast<float>(adam8_value(i, k, n));
            t.T[0][at]       = x;
            t.T[0][254 - at] = -x;
        }
    }
    t.T[0][255] = 1.0f;
    at          = 1;  // unsigned: 0, 254 positives, 1
    t.T[1][0]   = 0.0f;
    for (int i = 0; i < 7; ++i) {
        const int n = 2 << i;
        for (int k = 0; k < n; ++k, ++at) t.T[1][at] = static_cast<float>(adam8_value(i, k, n));
    }
    t.T[1][255] = 1.0f;
    for (int w = 0; w < 2; ++w) {
        t.E[w][0] = 0.0f;  // not a node
        for (int level = 0; level < 8; ++level) {
            for (int j = 0; j < (1 << level); ++j) {
                const int k = (2 * j + 1) * (128 >> level) - 1;  // the node's midpoint
                const double lo = t.T[w][k], hi = t.T[w][k + 1];
                t.E[w][(1 << level) + j] = static_cast<float>((lo + hi) / 2);
            }
        }
    }
    return t;
}

static const Adam8Tables h_adam8              = make_adam8_tables();
__device__ __constant__ Adam8Tables d_adam8 = make_adam8_tables();

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the workgroup's copy of the tables; every lane of a 256-lane block takes
// one entry of each
struct Adam8Lds {
    float T[2][256];
    float E[2][256];
};
__device__ __forceinline__ void adam8_load_tables(Adam8Lds &s)
{
    const int t = threadIdx.x;
    s.T[0][t]   = d_adam8.T[0][t];
    s.T[1][t]   = d_adam8.T[1][t];
    s.E[0][t]   = d_adam8.E[0][t];
    s.E[1][t]   = d_adam8.E[1][t];
    __syncthreads();
}

__device__ __forceinline__ unsigned adam8_key(float x)
{
    return (__float_as_uint(x) << 1) | (x >= 0.0f ? 1u : 0u);
}

// the maximum of k over the lane's row of 16, in every lane of the row
__device__ __forceinline__ unsigned adam8_row_max(unsigned k)
{
    // row_ror:8, 4, 2, 1
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0x128, 0xf, 0xf, false)));
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0x124, 0xf, 0xf, false)));
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0x122, 0xf, 0xf, false)));
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0x121, 0xf, 0xf, false)));
    return k;
}

// the block's signed scale from the row's key; a NaN anywhere gives 0x7FC00000
__device__ __forceinline__ float adam8_scale(unsigned key)
{
    const unsigned mag = key >> 1;
    if (mag > 0x7f800000u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float(mag | ((key & 1u) ? 0u : 0x80000000u));
}

__device__ __forceinline__ unsigned adam8_code(const float *E, float y)
{
    unsigned i = 1;
#pragma unroll
    for (int s = 0; s < 8; ++s) i = 2 * i + (E[i] < y ? 1u : 0u);
    return i & 255u;
}

// The lane's four elements of a block quantized: the dword of codes (element
// j in byte j) and the block's scale. Every lane of the row must be here.
__device__ __forceinline__ unsigned adam8_quantize4(const float (&x)[4], const float *E, float &a)
{
    unsigned key = max(max(adam8_key(x[0]), adam8_key(x[1])), max(adam8_key(x[2]), adam8_key(x[3])));
    a            = adam8_scale(adam8_row_max(key));
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float y = a == 0.0f ? 0.0f : __fdiv_rn(x[j], a);
        out |= adam8_code(E, y) << (8 * j);
    }
    return out;
}

__device__ __forceinline__ void adam8_dequantize4(unsigned codes, float a, const float *T,
                                                  float (&x)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = T[(codes >> (8 * j)) & 255u] * a;
}

// ---- the update ---------------------------------------------------------------
struct Adam8Seg {
    void *p16;      // the 16-bit parameters, written only (master kernels)
    const void *g;  // the summed gradients: f32, or 16-bit (master kernels)
    void *p;        // fp32: the parameters, or their master copy
    void *mc, *vc;  // codes, one byte per element
    void *ms, *vs;  // scales, one f32 per 64 elements
    size_t n;
    float w;  // ADAM_L2: weight_decay; ADAM_DECOUPLED: dk = 1 - lr*weight_decay
    float b1, c1, b2, c2, s2, eps, nss;
    int decay;
};
struct Adam8Args {
    Adam8Seg seg[kAdam8Seg];
    unsigned blk0[kAdam8Seg + 1];  // the search table (1-D grids only)
    int nseg;
};
static_assert(sizeof(Adam8Seg) == 104, "kernarg entry");
static_assert(sizeof(Adam8Args) + sizeof(Div) <= 3072, "kernarg budget");

// T = float: g is f32. T = bf16_t / f16_t: g is 16-bit and p16 is written.
template <typename T> struct Adam8Grad {
    using Raw = u32x2;
    template <int NT> __device__ static Raw load(const void *base, size_t ui)
    {
        const Raw *p = reinterpret_cast<const Raw *>(base) + ui;
        if constexpr (NT) return __builtin_nontemporal_load(p);
        else return *p;
    }
    __device__ static void widen(const Raw &r, f32x2 (&g)[2])
    {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if constexpr (std::is_same<T, bf16_t>::value) {
                g[w] = f32x2{__uint_as_float(r[w] << 16), __uint_as_float(r[w] & 0xffff0000u)};
            } else {
                g[w] = f32x2{SgdElt<T>::widen(static_cast<uint16_t>(r[w])),
                             SgdElt<T>::widen(static_cast<uint16_t>(r[w] >> 16))};
            }
        }
    }
};
template <> struct Adam8Grad<float> {
    using Raw = u32x4;
    template <int NT> __device__ static Raw load(const void *base, size_t ui)
    {
        return ld_u4<NT>(base, ui);
    }
    __device__ static void widen(const Raw &r, f32x2 (&g)[2])
    {
        g[0] = f32x2{__uint_as_float(r[0]), __uint_as_float(r[1])};
        g[1] = f32x2{__uint_as_float(r[2]), __uint_as_float(r[3])};
    }
};

// what one unit loads
template <typename T> struct Adam8Unit {
    typename Adam8Grad<T>::Raw g;
    u32x4 p;
    unsigned mc, vc;
    float ms, vs;
};

template <typename T>
__device__ __forceinline__ void adam8_load(const Adam8Seg &h, size_t ui, Adam8Unit<T> &r)
{
    r.g  = Adam8Grad<T>::template load<KF_ADAM8_G_NT>(h.g, ui);
    r.p  = ld_u4<0>(h.p, ui);
    r.mc = reinterpret_cast<const unsigned *>(h.mc)[ui];
    r.vc = reinterpret_cast<const unsigned *>(h.vc)[ui];
    r.ms = reinterpret_cast<const float *>(h.ms)[ui >> 4];
    r.vs = reinterpret_cast<const float *>(h.vs)[ui >> 4];
}

// one unit: p (and p16), both codes and, from the row's first lane, both
// scales updated and stored. Every lane of the row must be here.
template <typename T, int DIV, int DECAY, typename GATE>
__device__ __forceinline__ void adam8_unit(const Adam8Seg &h, const Div &d, size_t ui,
                                           const Adam8Unit<T> &r, const Adam8Lds &s,
                                           const GATE &gate)
{
    f32x2 p[2], g[2], m[2], v[2];
    float x[4];
    Adam8Grad<T>::widen(r.g, g);
    p[0] = f32x2{__uint_as_float(r.p[0]), __uint_as_float(r.p[1])};
    p[1] = f32x2{__uint_as_float(r.p[2]), __uint_as_float(r.p[3])};
    adam8_dequantize4(r.mc, r.ms, s.T[0], x);
    m[0] = f32x2{x[0], x[1]};
    m[1] = f32x2{x[2], x[3]};
    adam8_dequantize4(r.vc, r.vs, s.T[1], x);
    v[0] = f32x2{x[0], x[1]};
    v[1] = f32x2{x[2], x[3]};
    adam_math<float, DIV, DECAY, 2, f32x2>(p, g, m, v, h, d, gate);
    const u32x4 raw = {__float_as_uint(p[0].x), __float_as_uint(p[0].y), __float_as_uint(p[1].x),
                       __float_as_uint(p[1].y)};
    st_u4<0>(h.p, ui, raw);
    if constexpr (!std::is_same<T, float>::value) {
        u32x2 out;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            out[w] = static_cast<unsigned>(SgdElt<T>::narrow(p[w].x)) |
                     (static_cast<unsigned>(SgdElt<T>::narrow(p[w].y)) << 16);
        }
        reinterpret_cast<u32x2 *>(h.p16)[ui] = out;
    }
    const bool first = (threadIdx.x & 15) == 0;
    float a;
    const float xm[4] = {m[0].x, m[0].y, m[1].x, m[1].y};
    reinterpret_cast<unsigned *>(h.mc)[ui] = adam8_quantize4(xm, s.E[0], a);
    if (first) reinterpret_cast<float *>(h.ms)[ui >> 4] = a;
    const float xv[4] = {v[0].x, v[0].y, v[1].x, v[1].y};
    reinterpret_cast<unsigned *>(h.vc)[ui] = adam8_quantize4(xv, s.E[1], a);
    if (first) reinterpret_cast<float *>(h.vs)[ui >> 4] = a;
}

// Block `blk` of `nblk` on one segment. n is a multiple of 64, so the units
// are a multiple of 16 and a row is inside the segment or outside it as a
// whole: both conditions below are uniform over a row.
template <typename T, int DIV, int DECAY, typename GATE>
__device__ __forceinline__ void adam8_body(const Adam8Seg &h, const Div &d, size_t blk, size_t nblk,
                                           const Adam8Lds &s, const GATE &gate)
{
    constexpr int U = kAdam8Unroll, B = kAdam8Block;
    const size_t nunit  = h.n / kAdam8Elts;
    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nunit + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u0 = t * tile + threadIdx.x;
        if (u0 + (U - 1) * B < nunit) {
            // full tile: every load issued before the first use
            Adam8Unit<T> r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) adam8_load<T>(h, u0 + u * B, r[u]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) adam8_unit<T, DIV, DECAY>(h, d, u0 + u * B, r[u], s, gate);
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t ui = u0 + u * B;
                if (ui >= nunit) break;
                Adam8Unit<T> r;
                adam8_load<T>(h, ui, r);
                adam8_unit<T, DIV, DECAY>(h, d, ui, r, s, gate);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kAdam8Block) adam8_kernel(Adam8Args a, Div np, int div)
{
    __shared__ Adam8Lds s;
    adam8_load_tables(s);
    size_t blk, nblk;  // kf_update_batch.hpp's two grids
    const Adam8Seg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam8_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk, s,
                                                                        AdamNoGate{});
        });
    });
}

// adam8_kernel under a step gate (include/kungfu_amd.h
// kf_adam8_update_batch_gated): a skipped step returns before anything is
// loaded; otherwise grad_mul, s2 and nss come from device memory.
template <typename T>
__global__ void __launch_bounds__(kAdam8Block)
    adam8_gated_kernel(Adam8Args a, Div np, int div, const kf_step_gate *__restrict__ gate,
                       const kf_step_state *__restrict__ st)
{
    __shared__ Adam8Lds s;
    AdamGate<float> gt;
    if (adam_gate_load(gate, st, gt)) return;
    adam8_load_tables(s);
    size_t blk, nblk;
    const Adam8Seg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam8_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk, s, gt);
        });
    });
}

// ---- the quantizer alone --------------------------------------------------------
constexpr unsigned kAdam8CodecBlocks = 1024;  // beyond, the blocks stride

__global__ void __launch_bounds__(kAdam8Block)
    adam8_quantize_kernel(const void *__restrict__ src, void *__restrict__ codes,
                          void *__restrict__ scales, size_t nunit, int which)
{
    __shared__ Adam8Lds s;
    adam8_load_tables(s);
    const size_t stride = static_cast<size_t>(gridDim.x) * kAdam8Block;
    for (size_t ui = static_cast<size_t>(blockIdx.x) * kAdam8Block + threadIdx.x; ui < nunit;
         ui += stride) {
        const u32x4 r    = ld_u4<0>(src, ui);
        const float x[4] = {__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]),
                            __uint_as_float(r[3])};
        float a;
        reinterpret_cast<unsigned *>(codes)[ui] = adam8_quantize4(x, s.E[which], a);
        if ((threadIdx.x & 15) == 0) reinterpret_cast<float *>(scales)[ui >> 4] = a;
    }
}

__global__ void __launch_bounds__(kAdam8Block)
    adam8_dequantize_kernel(const void *__restrict__ codes, const void *__restrict__ scales,
                            void *__restrict__ dst, size_t nunit, int which)
{
    __shared__ Adam8Lds s;
    adam8_load_tables(s);
    const size_t stride = static_cast<size_t>(gridDim.x) * kAdam8Block;
    for (size_t ui = static_cast<size_t>(blockIdx.x) * kAdam8Block + threadIdx.x; ui < nunit;
         ui += stride) {
        float x[4];
        adam8_dequantize4(reinterpret_cast<const unsigned *>(codes)[ui],
                          reinterpret_cast<const float *>(scales)[ui >> 4], s.T[which], x);
        const u32x4 raw = {__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]),
                           __float_as_uint(x[3])};
        st_u4<0>(dst, ui, raw);
    }
}
}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail{"kf_adam8_update_batch"};
constexpr UpdateFail fail_gated{"kf_adam8_update_batch_gated"};
constexpr UpdateFail fail_master{"kf_adam8_master_update_batch"};
constexpr UpdateFail fail_master_gated{"kf_adam8_master_update_batch_gated"};
constexpr UpdateFail fail_quantize{"kf_adam8_quantize"};
constexpr UpdateFail fail_dequantize{"kf_adam8_dequantize"};

inline bool off4(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 4) != 0; }

// the tables of one call: params16 is null for the f32 entries
struct Adam8Tabs {
    void *const *params16;
    const void *const *grads;
    void *const *params;  // fp32: the parameters, or the masters
    void *const *m_codes, *const *v_codes, *const *m_scales, *const *v_scales;
};

// gate == nullptr: hyper[b] is segment b's and the parent kernel runs; else
// the one hyper[0] is every segment's and the gated kernel runs.
template <typename T>
int launch_adam8(const UpdateFail &fail, const Adam8Tabs &t, const size_t *counts, int nb, int np,
                 const kf_adam_hyper *hyper, hipStream_t s, const kf_step_gate *gate,
                 const kf_step_state *st)
{
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    return plan_update_batch<Adam8Args>(
        counts, nb, kAdam8Elts, static_cast<size_t>(kAdam8Block) * kAdam8Unroll,
        [&](Adam8Seg &g, int b) {
            g.p16 = t.params16 ? t.params16[b] : nullptr;
            g.g   = t.grads[b];
            g.p   = t.params[b];
            g.mc  = t.m_codes[b];
            g.vc  = t.v_codes[b];
            g.ms  = t.m_scales[b];
            g.vs  = t.v_scales[b];
            g.n   = counts[b];
            adam_scalars<float>(g, hyper[gate ? 0 : b]);
        },
        [&](unsigned gx, unsigned gy, const Adam8Args &a) {
            if (gate) {
                adam8_gated_kernel<T><<<dim3(gx, gy), kAdam8Block, 0, s>>>(a, dv, div, gate, st);
            } else {
                adam8_kernel<T><<<dim3(gx, gy), kAdam8Block, 0, s>>>(a, dv, div);
            }
            return launch_status(fail);
        });
}

// All four entries: every check comes before any HIP call.
int adam8_entry(const UpdateFail &fail, bool master, const Adam8Tabs &t, const size_t *counts,
                int nb, KungFu_Datatype dt, int np, const kf_adam_hyper *hyper, UpdateGate *g,
                void *stream)
{
    constexpr const char *off4_text  = "scales pointers must be 4-byte aligned";
    constexpr const char *off16_text =
        "parameter, gradient and codes pointers must be 16-byte aligned";
    const int rc = check_update_batch(
        fail, {{t.params16, 16, off16_text, !master}, {t.grads, 16, off16_text},
               {t.params, 16, off16_text}, {t.m_codes, 16, off16_text},
               {t.v_codes, 16, off16_text}, {t.m_scales, 4, off4_text},
               {t.v_scales, 4, off4_text}},
        {}, counts, nb, np, hyper, g, false,
        [&]() -> int {
            const bool half = dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16;
            if (master ? half : dt == KungFu_FLOAT) return KF_OK;
            return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE",
                        master ? "bf16 and f16 parameters only (f32 takes kf_adam8_update_batch)"
                               : "f32 only (bf16 and f16 take kf_adam8_master_update_batch)");
        },
        [&](int b) -> int {
            if (counts[b] % kAdam8Blk == 0) return KF_OK;
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "counts must be multiples of 64 (a block)");
        },
        no_check);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s              = static_cast<hipStream_t>(stream);
    const kf_step_gate *gate   = g ? g->gate : nullptr;
    const kf_step_state *state = g ? g->state : nullptr;
    if (dt == KungFu_FLOAT) return launch_adam8<float>(fail, t, counts, nb, np, hyper, s, gate, state);
    if (dt == KungFu_BFLOAT16) {
        return launch_adam8<bf16_t>(fail, t, counts, nb, np, hyper, s, gate, state);
    }
    return launch_adam8<f16_t>(fail, t, counts, nb, np, hyper, s, gate, state);
}

int codec_entry(const UpdateFail &fail, const void *f32, const void *codes, const void *scales,
                size_t n, int which, unsigned &grid)
{
    if (n == 0) return KF_OK;
    if (which != 0 && which != 1) return fail(KF_ERR_ARG, "KF_ERR_ARG", "which must be 0 or 1");
    if (n % kAdam8Blk) return fail(KF_ERR_ARG, "KF_ERR_ARG", "n must be a multiple of 64 (a block)");
    if (!f32 || !codes || !scales) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    if (off16(f32) || off16(codes)) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "value and codes pointers must be 16-byte aligned");
    }
    if (off4(scales)) return fail(KF_ERR_ARG, "KF_ERR_ARG", "the scales pointer must be 4-byte aligned");
    const size_t blocks = (n / kAdam8Elts + kAdam8Block - 1) / kAdam8Block;
    grid = static_cast<unsigned>(blocks < kAdam8CodecBlocks ? blocks : kAdam8CodecBlocks);
    return KF_OK;
}

}  // namespace

extern "C" {

int kf_adam8_codebook(int which, float *out)
{
    constexpr UpdateFail fail_book{"kf_adam8_codebook"};
    if (which != 0 && which != 1) return fail_book(KF_ERR_ARG, "KF_ERR_ARG", "which must be 0 or 1");
    if (!out) return fail_book(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    for (int k = 0; k < 256; ++k) out[k] = h_adam8.T[which][k];
    return KF_OK;
}

int kf_adam8_update_batch(void *const *params, const void *const *grads, void *const *m_codes,
                          void *const *v_codes, void *const *m_scales, void *const *v_scales,
                          const size_t *counts, int nb, KungFu_Datatype dt, int np,
                          const kf_adam_hyper *hyper, void *stream)
{
    const Adam8Tabs t = {nullptr, grads, params, m_codes, v_codes, m_scales, v_scales};
    return adam8_entry(fail, false, t, counts, nb, dt, np, hyper, nullptr, stream);
}

int kf_adam8_update_batch_gated(void *const *params, const void *const *grads,
                                void *const *m_codes, void *const *v_codes,
                                void *const *m_scales, void *const *v_scales,
                                const size_t *counts, int nb, KungFu_Datatype dt, int np,
                                const kf_adam_hyper *hyper, const kf_step_gate *gate,
                                const kf_step_state *state, void *stream)
{
    const Adam8Tabs t = {nullptr, grads, params, m_codes, v_codes, m_scales, v_scales};
    UpdateGate g = {gate, state, {}};
    return adam8_entry(fail_gated, false, t, counts, nb, dt, np, hyper, &g, stream);
}

int kf_adam8_master_update_batch(void *const *params16, const void *const *grads16,
                                 void *const *masters, void *const *m_codes, void *const *v_codes,
                                 void *const *m_scales, void *const *v_scales,
                                 const size_t *counts, int nb, KungFu_Datatype dt, int np,
                                 const kf_adam_hyper *hyper, void *stream)
{
    const Adam8Tabs t = {params16, grads16, masters, m_codes, v_codes, m_scales, v_scales};
    return adam8_entry(fail_master, true, t, counts, nb, dt, np, hyper, nullptr, stream);
}

int kf_adam8_master_update_batch_gated(void *const *params16, const void *const *grads16,
                                       void *const *masters, void *const *m_codes,
                                       void *const *v_codes, void *const *m_scales,
                                       void *const *v_scales, const size_t *counts, int nb,
                                       KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                       const kf_step_gate *gate, const kf_step_state *state,
                                       void *stream)
{
    const Adam8Tabs t = {params16, grads16, masters, m_codes, v_codes, m_scales, v_scales};
    UpdateGate g = {gate, state, {}};
    return adam8_entry(fail_master_gated, true, t, counts, nb, dt, np, hyper, &g, stream);
}

int kf_adam8_quantize(const void *src, void *codes, void *scales, size_t n, int which,
                      void *stream)
{
    unsigned grid = 0;
    const int rc  = codec_entry(fail_quantize, src, codes, scales, n, which, grid);
    if (rc != KF_OK || n == 0) return rc;
    adam8_quantize_kernel<<<grid, kAdam8Block, 0, static_cast<hipStream_t>(stream)>>>(
        src, codes, scales, n / kAdam8Elts, which);
    return launch_status(fail_quantize);
}

int kf_adam8_dequantize(const void *codes, const void *scales, void *dst, size_t n, int which,
                        void *stream)
{
    unsigned grid = 0;
    const int rc  = codec_entry(fail_dequantize, dst, codes, scales, n, which, grid);
    if (rc != KF_OK || n == 0) return rc;
    adam8_dequantize_kernel<<<grid, kAdam8Block, 0, static_cast<hipStream_t>(stream)>>>(
        codes, scales, dst, n / kAdam8Elts, which);
    return launch_status(fail_dequantize);
}

}  // extern "C"
