// kf_adam_master.hip — the Adam / AdamW update of 16-bit parameters through an
// fp32 master copy and fp32 state (include/kungfu_amd.h
// kf_adam_master_update_batch):
//
//   reduce-scatter(grads16) -> [own shard: widen g, kf_adam.hip's f32 update
//                               on (master, g, m, v), p16 = narrow(master)]
//                           -> all-gather(params16)
//
// kf_adam.hip's shape: one batched element-wise launch over up to
// kAdamMasterSeg segments, every segment with its own pointers, count and
// scalars in the kernarg segment (the launch planner and the segment lookup
// are kf_update_batch.hpp's). A segment reads g (2 B) and master, m, v
// (12 B) and writes master, m, v (12 B) and p16 (2 B): 28 bytes per element,
// the f32 kernel's 7 x 4. The old 16-bit parameter value is never read.
//
// Arithmetic: adam_math<float, ...> of kf_adam_math.hpp, the f32 kernel's own,
// on the widened gradient (the widening is exact); the /np is the fp32 one and
// is not rounded to 16 bits. The only rounding to 16 bits is the last:
// p16 = narrow(master'), round-to-nearest-even (SgdElt<T>::narrow). The
// narrowed value is a sum, so f16's v_fma_mixlo_f16 -0 hazard (kf_sgd_elt.hpp)
// does not arise; tests/test_sharded_adam_master_gpu.py's narrowing grid
// checks both zeros.
//
// One unit is kAdamMasterElts consecutive elements of a lane. 4 (the default):
// an 8-byte access on the 16-bit streams and one 16-byte access on each fp32
// stream, so every wave instruction is contiguous. 8: one 16-byte access on
// the 16-bit streams and two 16-byte accesses, 32 bytes apart per lane, on
// each fp32 stream. DESIGN.md §15 has both measured.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_adam_math.hpp"
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal: kf_adam.hip's. g is
// dead after this kernel; master, m and v are read and written in place; p16
// is what the all-gather sends next.
#ifndef KF_ADAM_MASTER_G_NT
#define KF_ADAM_MASTER_G_NT 1
#endif
#ifndef KF_ADAM_MASTER_WMV_NT
#define KF_ADAM_MASTER_WMV_NT 0
#endif
#ifndef KF_ADAM_MASTER_ST_NT
#define KF_ADAM_MASTER_ST_NT 0
#endif

namespace kf
{
constexpr int kAdamMasterSeg   = 32;
constexpr int kAdamMasterBlock = 256;
#ifndef KF_ADAM_MASTER_ELTS
#define KF_ADAM_MASTER_ELTS 4  // elements per unit: 4 or 8
#endif
constexpr int kAdamMasterElts = KF_ADAM_MASTER_ELTS;
static_assert(kAdamMasterElts == 4 || kAdamMasterElts == 8, "a unit is 4 or 8 elements");
// Units per lane per tile. A unit's loads are 3.5 (4 elements) or 7 (8
// elements) 16-byte equivalents, so 14 are in flight per lane where
// kf_adam.hip has 16.
#ifndef KF_ADAM_MASTER_UNROLL
#define KF_ADAM_MASTER_UNROLL (16 / KF_ADAM_MASTER_ELTS)
#endif
constexpr int kAdamMasterUnroll = KF_ADAM_MASTER_UNROLL;

struct AdamMasterSeg {
    void *p16;      // the 16-bit parameters, written only
    const void *g;  // the 16-bit summed gradients
    void *p, *m, *v;  // fp32: master, exp_avg, exp_avg_sq
    size_t n;
    float w;  // ADAM_L2: weight_decay; ADAM_DECOUPLED: dk = 1 - lr*weight_decay
    float b1, c1, b2, c2, s2, eps, nss;
    int decay;
};
struct AdamMasterArgs {
    AdamMasterSeg seg[kAdamMasterSeg];
    unsigned blk0[kAdamMasterSeg + 1];  // the search table (1-D grids only)
    int nseg;
};
// kf_adam.hip's budget: an entry is 88 bytes (one pointer more than
// AdamSeg<float>'s 80), so 32 of them; 33 would be 3,076 bytes
static_assert(sizeof(AdamMasterSeg) == 88, "kernarg entry");
static_assert(sizeof(AdamMasterArgs) + sizeof(Div) <= 3072, "kernarg budget");
static_assert(sizeof(AdamMasterArgs) + sizeof(AdamMasterSeg) + 4 + sizeof(Div) > 3072,
              "kAdamMasterSeg is the most the budget holds");

constexpr int kMH = kAdamMasterElts / 2;  // lane pairs (and 16-bit words) per unit
constexpr int kMK = kAdamMasterElts / 4;  // 16-byte fp32 vectors per stream per unit
typedef unsigned int u32xh __attribute__((ext_vector_type(kMH)));  // a unit of a 16-bit stream

template <int NT> __device__ __forceinline__ u32xh ld_h(const void *base, size_t ui)
{
    const u32xh *p = reinterpret_cast<const u32xh *>(base) + ui;
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// two 16-bit lanes of a 32-bit word <-> a lane pair
template <typename T> __device__ __forceinline__ f32x2 widen2(unsigned w)
{
    if constexpr (std::is_same<T, bf16_t>::value) {
        return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
    } else {
        return f32x2{SgdElt<T>::widen(static_cast<uint16_t>(w)),
                     SgdElt<T>::widen(static_cast<uint16_t>(w >> 16))};
    }
}
template <typename T> __device__ __forceinline__ unsigned narrow2(f32x2 x)
{
    return static_cast<unsigned>(SgdElt<T>::narrow(x.x)) |
           (static_cast<unsigned>(SgdElt<T>::narrow(x.y)) << 16);
}

__device__ __forceinline__ void unpack_f32(const u32x4 (&raw)[kMK], f32x2 (&x)[kMH])
{
#pragma unroll
    for (int j = 0; j < kMK; ++j) {
        x[2 * j]     = f32x2{__uint_as_float(raw[j][0]), __uint_as_float(raw[j][1])};
        x[2 * j + 1] = f32x2{__uint_as_float(raw[j][2]), __uint_as_float(raw[j][3])};
    }
}
__device__ __forceinline__ void store_f32(void *base, size_t ui, const f32x2 (&x)[kMH])
{
#pragma unroll
    for (int j = 0; j < kMK; ++j) {
        const u32x4 raw = {__float_as_uint(x[2 * j].x), __float_as_uint(x[2 * j].y),
                           __float_as_uint(x[2 * j + 1].x), __float_as_uint(x[2 * j + 1].y)};
        st_u4<KF_ADAM_MASTER_ST_NT>(base, ui * kMK + j, raw);
    }
}

// one unit: master, m, v and the narrowed parameters updated and stored
template <typename T, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void master_unit(const AdamMasterSeg &h, const Div &d, size_t ui,
                                            const u32xh &rg, const u32x4 (&rp)[kMK],
                                            const u32x4 (&rm)[kMK], const u32x4 (&rv)[kMK],
                                            const GATE &gate = GATE{})
{
    f32x2 p[kMH], g[kMH], m[kMH], v[kMH];
#pragma unroll
    for (int w = 0; w < kMH; ++w) g[w] = widen2<T>(rg[w]);
    unpack_f32(rp, p);
    unpack_f32(rm, m);
    unpack_f32(rv, v);
    adam_math<float, DIV, DECAY, kMH, f32x2>(p, g, m, v, h, d, gate);
    store_f32(h.p, ui, p);
    store_f32(h.m, ui, m);
    store_f32(h.v, ui, v);
    u32xh out;
#pragma unroll
    for (int w = 0; w < kMH; ++w) out[w] = narrow2<T>(p[w]);
    u32xh *dst = reinterpret_cast<u32xh *>(h.p16) + ui;
    if constexpr (KF_ADAM_MASTER_ST_NT) __builtin_nontemporal_store(out, dst);
    else *dst = out;
}

template <int NT>
__device__ __forceinline__ void ld_f32(const void *base, size_t ui, u32x4 (&raw)[kMK])
{
#pragma unroll
    for (int j = 0; j < kMK; ++j) raw[j] = ld_u4<NT>(base, ui * kMK + j);
}

// Block `blk` of `nblk` on one segment.
template <typename T, int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void master_body(const AdamMasterSeg &h, const Div &d, size_t blk,
                                            size_t nblk, const GATE &gate = GATE{})
{
    using E         = SgdElt<T>;
    constexpr int N = kAdamMasterElts;
    constexpr int U = kAdamMasterUnroll, B = kAdamMasterBlock;
    constexpr int WNT = KF_ADAM_MASTER_WMV_NT;
    const size_t n     = h.n;
    const size_t nunit = n / N;

    // the scalar tail: fewer than N elements, on the segment's first block
    const size_t ti = nunit * N + threadIdx.x;
    if (blk == 0 && ti < n) {
        uint16_t *s16       = reinterpret_cast<uint16_t *>(h.p16);
        const uint16_t *sg  = reinterpret_cast<const uint16_t *>(h.g);
        float *sp = reinterpret_cast<float *>(h.p), *sm = reinterpret_cast<float *>(h.m);
        float *sv = reinterpret_cast<float *>(h.v);
        float p[1] = {sp[ti]}, g[1] = {E::widen(sg[ti])}, m[1] = {sm[ti]}, v[1] = {sv[ti]};
        adam_math<float, DIV, DECAY, 1, float>(p, g, m, v, h, d, gate);
        sp[ti]  = p[0];
        sm[ti]  = m[0];
        sv[ti]  = v[0];
        s16[ti] = E::narrow(p[0]);
    }

    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nunit + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u0 = t * tile + threadIdx.x;
        if (u0 + (U - 1) * B < nunit) {
            // full tile: every load issued before the first use
            u32xh rg[U];
            u32x4 rp[U][kMK], rm[U][kMK], rv[U][kMK];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = ld_h<KF_ADAM_MASTER_G_NT>(h.g, u0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) ld_f32<WNT>(h.p, u0 + u * B, rp[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) ld_f32<WNT>(h.m, u0 + u * B, rm[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) ld_f32<WNT>(h.v, u0 + u * B, rv[u]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                master_unit<T, DIV, DECAY>(h, d, u0 + u * B, rg[u], rp[u], rm[u], rv[u], gate);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t ui = u0 + u * B;
                if (ui >= nunit) break;
                const u32xh rg = ld_h<KF_ADAM_MASTER_G_NT>(h.g, ui);
                u32x4 rp[kMK], rm[kMK], rv[kMK];
                ld_f32<WNT>(h.p, ui, rp);
                ld_f32<WNT>(h.m, ui, rm);
                ld_f32<WNT>(h.v, ui, rv);
                master_unit<T, DIV, DECAY>(h, d, ui, rg, rp, rm, rv, gate);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kAdamMasterBlock)
    adam_master_kernel(AdamMasterArgs a, Div np, int div)
{
    size_t blk, nblk;  // kf_update_batch.hpp's two grids
    const AdamMasterSeg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            master_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk);
        });
    });
}

// adam_master_kernel under a step gate (include/kungfu_amd.h
// kf_adam_master_update_batch_gated): a skipped step returns before anything
// is loaded; otherwise grad_mul, s2 and nss come from device memory.
template <typename T>
__global__ void __launch_bounds__(kAdamMasterBlock)
    adam_master_gated_kernel(AdamMasterArgs a, Div np, int div,
                             const kf_step_gate *__restrict__ gate,
                             const kf_step_state *__restrict__ st)
{
    AdamGate<float> gt;
    if (adam_gate_load(gate, st, gt)) return;
    size_t blk, nblk;
    const AdamMasterSeg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            master_body<T, decltype(DIV)::value, decltype(DECAY)::value>(g, np, blk, nblk, gt);
        });
    });
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail{"kf_adam_master_update_batch"};
constexpr UpdateFail fail_gated{"kf_adam_master_update_batch_gated"};

// gate == nullptr: hyper[b] is segment b's and the parent kernel runs; else
// the one hyper[0] is every segment's and the gated kernel runs.
template <typename T>
int launch_master(void *const *params16, const void *const *grads16, void *const *masters,
                  void *const *ms, void *const *vs, const size_t *counts, int nb, int np,
                  const kf_adam_hyper *hyper, hipStream_t s, const kf_step_gate *gate = nullptr,
                  const kf_step_state *st = nullptr)
{
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    return plan_update_batch<AdamMasterArgs>(
        counts, nb, kAdamMasterElts, static_cast<size_t>(kAdamMasterBlock) * kAdamMasterUnroll,
        [&](AdamMasterSeg &g, int b) {
            g.p16 = params16[b];
            g.g   = grads16[b];
            g.p   = masters[b];
            g.m   = ms[b];
            g.v   = vs[b];
            g.n   = counts[b];
            adam_scalars<float>(g, hyper[gate ? 0 : b]);
        },
        [&](unsigned gx, unsigned gy, const AdamMasterArgs &a) {
            if (gate) {
                adam_master_gated_kernel<T>
                    <<<dim3(gx, gy), kAdamMasterBlock, 0, s>>>(a, dv, div, gate, st);
                return launch_status(fail_gated);
            }
            adam_master_kernel<T><<<dim3(gx, gy), kAdamMasterBlock, 0, s>>>(a, dv, div);
            return launch_status(fail);
        });
}

// Both entries: every check comes before any HIP call.
int master_entry(const UpdateFail &fail, void *const *params16, const void *const *grads16,
                 void *const *masters, void *const *exp_avgs, void *const *exp_avg_sqs,
                 const size_t *counts, int nb, KungFu_Datatype dt, int np,
                 const kf_adam_hyper *hyper, UpdateGate *g, void *stream)
{
    const int rc = check_update_batch(
        fail, {{params16, 16, kOff16}, {grads16, 16, kOff16}, {masters, 16, kOff16},
               {exp_avgs, 16, kOff16}, {exp_avg_sqs, 16, kOff16}},
        {}, counts, nb, np, hyper, g, false,
        [&]() -> int {
            if (dt == KungFu_BFLOAT16 || dt == KungFu_FLOAT16) return KF_OK;
            return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE",
                        "bf16 and f16 parameters only (f32 and f64 take kf_adam_update_batch)");
        },
        no_check, no_check);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s              = static_cast<hipStream_t>(stream);
    const kf_step_gate *gate   = g ? g->gate : nullptr;
    const kf_step_state *state = g ? g->state : nullptr;
    if (dt == KungFu_BFLOAT16) {
        return launch_master<bf16_t>(params16, grads16, masters, exp_avgs, exp_avg_sqs, counts, nb,
                                     np, hyper, s, gate, state);
    }
    return launch_master<f16_t>(params16, grads16, masters, exp_avgs, exp_avg_sqs, counts, nb, np,
                                hyper, s, gate, state);
}

}  // namespace

extern "C" {

int kf_adam_master_update_batch(void *const *params16, const void *const *grads16,
                                void *const *masters, void *const *exp_avgs,
                                void *const *exp_avg_sqs, const size_t *counts, int nb,
                                KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                void *stream)
{
    return master_entry(fail, params16, grads16, masters, exp_avgs, exp_avg_sqs, counts, nb, dt, np,
                        hyper, nullptr, stream);
}

int kf_adam_master_update_batch_gated(void *const *params16, const void *const *grads16,
                                      void *const *masters, void *const *exp_avgs,
                                      void *const *exp_avg_sqs, const size_t *counts, int nb,
                                      KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                      const kf_step_gate *gate, const kf_step_state *state,
                                      void *stream)
{
    UpdateGate g = {gate, state, {}};
    return master_entry(fail_gated, params16, grads16, masters, exp_avgs, exp_avg_sqs, counts, nb,
                        dt, np, hyper, &g, stream);
}

}  // extern "C"
