// kf_adam_sr.hip — the Adam / AdamW update of bf16 parameters with bf16 state,
// fp32 arithmetic in registers and stochastic rounding where a value is
// narrowed back to bf16 (include/kungfu_amd.h kf_adam_sr_update_batch,
// DESIGN.md §18):
//
//   reduce-scatter(grads) -> [own shard: widen p, g, m, v; kf_adam.hip's f32
//                             update; p = sr(p'), m = rne(m'), v = sr(v')]
//                         -> all-gather(params)
//
// kf_adam.hip's shape and traffic: one batched element-wise launch over up to
// kAdamSrSeg segments, every segment with its own pointers, count, scalars,
// element base and stream word in the kernarg segment (the launch planner and
// the segment lookup are kf_update_batch.hpp's). A segment reads g, p, m and v
// once and writes p, m and v once, 2 bytes each: 14 bytes per element.
//
// Arithmetic: adam_math<float, ...> of kf_adam_math.hpp, the f32 kernel's own,
// on the widened values (the widening is exact); the /np is the fp32 one and
// nothing in between is rounded to 16 bits, as in kf_adam_master.hip.
//
// Narrowing. sr(x, r) of a finite x with 16 random bits r is
// (bits(x) + r) >> 16 in unsigned 32-bit arithmetic: the value goes to the bf16
// above (in magnitude) with probability low16(x) / 2^16 and is truncated
// otherwise, so E[sr(x)] = x; an x that is a bf16 already is returned whatever
// r is; a carry into the exponent is kept, so the largest binade may round to
// inf. inf and NaN narrow as f32_to_bf16 does. Plain integer code: the
// hardware convert was not taken.
//
// Random bits: a pure function of (key, stream word, element index e = base +
// i), one Philox2x32-10 evaluation per element pair:
//   (a, b) = philox2x32_10(c0 = (uint32)(e >> 1), c1 = stream, key)
//   w = (e & 1) ? b : a;  r_p = w >> 16;  r_v = w & 0xffff
// base is a multiple of 8, so a 16-byte vector's four 32-bit words are four
// pairs (2k, 2k + 1): word k of vector vi has c0 = (base >> 1) + 4 * vi + k, its
// low lane takes a and its high lane b. Launch geometry, the segment split,
// rank and world play no part.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_adam_math.hpp"
#include "kf_update_batch.hpp"

// Load / store policy of the streams, 1 = non-temporal: kf_adam.hip's. g is
// dead after this kernel; p, m and v are read and written in place.
#ifndef KF_ADAM_SR_G_NT
#define KF_ADAM_SR_G_NT 1
#endif
#ifndef KF_ADAM_SR_PMV_NT
#define KF_ADAM_SR_PMV_NT 0
#endif
#ifndef KF_ADAM_SR_ST_NT
#define KF_ADAM_SR_ST_NT 0
#endif

namespace kf
{
constexpr int kAdamSrSeg   = 32;
constexpr int kAdamSrBlock = 256;
#ifndef KF_ADAM_SR_UNROLL
#define KF_ADAM_SR_UNROLL 4  // 16-B vectors per lane per stream per tile
#endif
constexpr int kAdamSrUnroll = KF_ADAM_SR_UNROLL;
constexpr int kAdamSrElts   = 8;  // bf16 elements of a 16-byte vector

struct AdamSrSeg {
    void *p;
    const void *g;
    void *m, *v;
    size_t n;
    uint64_t base;  // element index of the segment's first element, a multiple of 8
    float w;        // ADAM_L2: weight_decay; ADAM_DECOUPLED: dk = 1 - lr*weight_decay
    float b1, c1, b2, c2, s2, eps, nss;
    int decay;
    uint32_t stream;  // Philox counter word c1
};
struct AdamSrArgs {
    AdamSrSeg seg[kAdamSrSeg];
    unsigned blk0[kAdamSrSeg + 1];  // the search table (1-D grids only)
    int nseg;
};
// kf_adam.hip's budget: an entry is 88 bytes (AdamSeg<float>'s 80, the base
// and the stream word in what was padding), so 32 of them; the Philox key is
// a kernel argument of its own beside np
static_assert(sizeof(AdamSrSeg) == 88, "kernarg entry");
static_assert(sizeof(AdamSrArgs) + sizeof(Div) + sizeof(uint32_t) <= 3072, "kernarg budget");
static_assert(sizeof(AdamSrArgs) + sizeof(AdamSrSeg) + 4 + sizeof(Div) + sizeof(uint32_t) > 3072,
              "kAdamSrSeg is the most the budget holds");

// Philox2x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
// 3"): ten rounds of {hi(M * c0) ^ key ^ c1, lo(M * c0)}, the key bumped by
// the golden ratio between rounds. The key sequence is wave-uniform.
struct Philox2 {
    uint32_t a, b;
};
// hi ^ key ^ c1 as one three-input bit operation where the target has one
// (truth table 0x96); key is wave-uniform.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
__device__ __forceinline__ Philox2 philox2x32_10(uint32_t c0, uint32_t c1, uint32_t key)
{
    constexpr uint32_t M = 0xD256D193u, W = 0x9E3779B9u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t prod = static_cast<uint64_t>(M) * c0;
        c0 = xor3(static_cast<uint32_t>(prod >> 32), key, c1);
        c1 = static_cast<uint32_t>(prod);
        key += W;
    }
    return Philox2{c0, c1};
}

// sr(x, rx) in the low half and sr(y, ry) in the high half of one word,
// rx, ry < 2^16: the header comment's narrowing, without a branch. A finite
// |x| is at most 0x7f7fffff, so adding r never reaches the sign bit. inf and
// NaN take their halves of the round-to-nearest narrowing of the pair (one
// v_cvt_pk_bf16_f32: inf stays, a NaN is made quiet).
__device__ __forceinline__ uint32_t sr_pair(float x, float y, uint32_t rx, uint32_t ry)
{
    const uint32_t sx = __float_as_uint(x) + rx, sy = __float_as_uint(y) + ry;
    const uint32_t sr  = (sx >> 16) | (sy & 0xffff0000u);
    const uint32_t rne = static_cast<uint32_t>(f32_to_bf16(x)) |
                         (static_cast<uint32_t>(f32_to_bf16(y)) << 16);
    const uint32_t mask = (__builtin_isfinite(x) ? 0x0000ffffu : 0u) |
                          (__builtin_isfinite(y) ? 0xffff0000u : 0u);
    return (sr & mask) | (rne & ~mask);
}

// one vector: p, m and v updated, narrowed and stored
template <int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void adam_sr_vec(const AdamSrSeg &h, const Div &d, uint32_t key,
                                            size_t vi, const u32x4 &rp, const u32x4 &rg,
                                            const u32x4 &rm, const u32x4 &rv,
                                            const GATE &gate = GATE{})
{
    using SV        = SgdVec<bf16_t>;
    constexpr int H = SV::N / 2;
    f32x2 p[H], g[H], m[H], v[H];
    SV::unpack(rp, p);
    SV::unpack(rg, g);
    SV::unpack(rm, m);
    SV::unpack(rv, v);
    adam_math<float, DIV, DECAY, H, f32x2>(p, g, m, v, h, d, gate);
    // every valid element index is below 2^33, so its pair index fits 32 bits
    const uint32_t c0 = static_cast<uint32_t>(h.base >> 1) + static_cast<uint32_t>(vi) * H;
    u32x4 op, om, ov;
#pragma unroll
    for (int w = 0; w < H; ++w) {
        const Philox2 x = philox2x32_10(c0 + w, h.stream, key);
        op[w] = sr_pair(p[w].x, p[w].y, x.a >> 16, x.b >> 16);
        om[w] = static_cast<uint32_t>(f32_to_bf16(m[w].x)) |
                (static_cast<uint32_t>(f32_to_bf16(m[w].y)) << 16);
        ov[w] = sr_pair(v[w].x, v[w].y, x.a & 0xffffu, x.b & 0xffffu);
    }
    st_u4<KF_ADAM_SR_ST_NT>(h.p, vi, op);
    st_u4<KF_ADAM_SR_ST_NT>(h.m, vi, om);
    st_u4<KF_ADAM_SR_ST_NT>(h.v, vi, ov);
}

// Block `blk` of `nblk` on one segment.
template <int DIV, int DECAY, typename GATE = AdamNoGate>
__device__ __forceinline__ void adam_sr_body(const AdamSrSeg &h, const Div &d, uint32_t key,
                                             size_t blk, size_t nblk, const GATE &gate = GATE{})
{
    constexpr int N = kAdamSrElts;
    constexpr int U = kAdamSrUnroll, B = kAdamSrBlock;
    constexpr int PNT = KF_ADAM_SR_PMV_NT;
    const size_t n    = h.n;
    const size_t nvec = n / N;

    // the scalar tail: fewer than N elements, on the segment's first block
    const size_t ti = nvec * N + threadIdx.x;
    if (blk == 0 && ti < n) {
        uint16_t *sp       = reinterpret_cast<uint16_t *>(h.p);
        const uint16_t *sq = reinterpret_cast<const uint16_t *>(h.g);
        uint16_t *sm       = reinterpret_cast<uint16_t *>(h.m);
        uint16_t *sv       = reinterpret_cast<uint16_t *>(h.v);
        float p[1] = {bf16_to_f32(sp[ti])}, g[1] = {bf16_to_f32(sq[ti])};
        float m[1] = {bf16_to_f32(sm[ti])}, v[1] = {bf16_to_f32(sv[ti])};
        adam_math<float, DIV, DECAY, 1, float>(p, g, m, v, h, d, gate);
        const uint64_t e = h.base + ti;
        const Philox2 x  = philox2x32_10(static_cast<uint32_t>(e >> 1), h.stream, key);
        const uint32_t w = (e & 1) ? x.b : x.a;
        // the one narrowing there is: both halves of a pair hold this element
        sp[ti] = static_cast<uint16_t>(sr_pair(p[0], p[0], w >> 16, w >> 16));
        sm[ti] = f32_to_bf16(m[0]);
        sv[ti] = static_cast<uint16_t>(sr_pair(v[0], v[0], w & 0xffffu, w & 0xffffu));
    }

    const size_t tile   = static_cast<size_t>(B) * U;
    const size_t ntiles = (nvec + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        if (v0 + (U - 1) * B < nvec) {
            // full tile: every load issued before the first use
            u32x4 rp[U], rg[U], rm[U], rv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rg[u] = ld_u4<KF_ADAM_SR_G_NT>(h.g, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rp[u] = ld_u4<PNT>(h.p, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rm[u] = ld_u4<PNT>(h.m, v0 + u * B);
#pragma unroll
            for (int u = 0; u < U; ++u) rv[u] = ld_u4<PNT>(h.v, v0 + u * B);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                adam_sr_vec<DIV, DECAY>(h, d, key, v0 + u * B, rp[u], rg[u], rm[u], rv[u], gate);
            }
        } else {
            // ragged last tile
            for (int u = 0; u < U; ++u) {
                const size_t vi = v0 + u * B;
                if (vi >= nvec) break;
                const u32x4 rg = ld_u4<KF_ADAM_SR_G_NT>(h.g, vi), rp = ld_u4<PNT>(h.p, vi);
                const u32x4 rm = ld_u4<PNT>(h.m, vi), rv = ld_u4<PNT>(h.v, vi);
                adam_sr_vec<DIV, DECAY>(h, d, key, vi, rp, rg, rm, rv, gate);
            }
        }
    }
}

// T is bf16_t alone; the template keeps the kernels' names in the siblings'
// form (tests/test_sharded_adam_sr_isa.py reads the dtype from them).
template <typename T>
__global__ void __launch_bounds__(kAdamSrBlock)
    adam_sr_kernel(AdamSrArgs a, Div np, int div, uint32_t key)
{
    static_assert(std::is_same<T, bf16_t>::value, "bf16 only");
    size_t blk, nblk;  // kf_update_batch.hpp's two grids
    const AdamSrSeg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam_sr_body<decltype(DIV)::value, decltype(DECAY)::value>(g, np, key, blk, nblk);
        });
    });
}

// adam_sr_kernel under a step gate (include/kungfu_amd.h
// kf_adam_sr_update_batch_gated): a skipped step returns before anything is
// loaded; otherwise grad_mul, s2 and nss come from device memory.
template <typename T>
__global__ void __launch_bounds__(kAdamSrBlock)
    adam_sr_gated_kernel(AdamSrArgs a, Div np, int div, uint32_t key,
                         const kf_step_gate *__restrict__ gate,
                         const kf_step_state *__restrict__ st)
{
    static_assert(std::is_same<T, bf16_t>::value, "bf16 only");
    AdamGate<float> gt;
    if (adam_gate_load(gate, st, gt)) return;
    size_t blk, nblk;
    const AdamSrSeg &g = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto DIV) {
        dispatch_decay(g.decay, [&](auto DECAY) {
            adam_sr_body<decltype(DIV)::value, decltype(DECAY)::value>(g, np, key, blk, nblk, gt);
        });
    });
}

// The narrowing alone on n values with given random bits, two values to a
// lane as in the update: what the GPU sweep of
// tests/test_sharded_adam_sr_gpu.py runs against the restatement.
__global__ void __launch_bounds__(256)
    adam_sr_narrow_kernel(const uint32_t *__restrict__ x, const uint16_t *__restrict__ r,
                          uint16_t *__restrict__ out, size_t n)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t pairs  = (n + 1) / 2;
    for (size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < pairs;
         j += stride) {
        const size_t i0 = 2 * j, i1 = i0 + 1 < n ? i0 + 1 : i0;
        const uint32_t w = sr_pair(__uint_as_float(x[i0]), __uint_as_float(x[i1]), r[i0], r[i1]);
        out[i0] = static_cast<uint16_t>(w);
        if (i1 != i0) out[i1] = static_cast<uint16_t>(w >> 16);
    }
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail{"kf_adam_sr_update_batch"};
constexpr UpdateFail fail_gated{"kf_adam_sr_update_batch_gated"};
constexpr UpdateFail fail_narrow{"kf_adam_sr_narrow"};

constexpr uint64_t kMaxElement = 1ull << 33;  // a pair index is 32 bits

// gate == nullptr: hyper[b] is segment b's and the parent kernel runs; else
// the one hyper[0] is every segment's and the gated kernel runs.
int launch_adam_sr(void *const *params, const void *const *grads, void *const *ms,
                   void *const *vs, const size_t *counts, const uint64_t *bases,
                   const uint32_t *streams, int nb, int np, const kf_adam_hyper *hyper,
                   uint32_t key, hipStream_t s, const kf_step_gate *gate, const kf_step_state *st)
{
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    return plan_update_batch<AdamSrArgs>(
        counts, nb, kAdamSrElts, static_cast<size_t>(kAdamSrBlock) * kAdamSrUnroll,
        [&](AdamSrSeg &g, int b) {
            g.p      = params[b];
            g.g      = grads[b];
            g.m      = ms[b];
            g.v      = vs[b];
            g.n      = counts[b];
            g.base   = bases[b];
            g.stream = streams[b];
            adam_scalars<float>(g, hyper[gate ? 0 : b]);
        },
        [&](unsigned gx, unsigned gy, const AdamSrArgs &a) {
            if (gate) {
                adam_sr_gated_kernel<bf16_t>
                    <<<dim3(gx, gy), kAdamSrBlock, 0, s>>>(a, dv, div, key, gate, st);
                return launch_status(fail_gated);
            }
            adam_sr_kernel<bf16_t><<<dim3(gx, gy), kAdamSrBlock, 0, s>>>(a, dv, div, key);
            return launch_status(fail);
        });
}

// Both entries: every check comes before any HIP call.
int adam_sr_entry(const UpdateFail &fail, void *const *params, const void *const *grads,
                  void *const *exp_avgs, void *const *exp_avg_sqs, const size_t *counts,
                  const uint64_t *bases, const uint32_t *streams, int nb, KungFu_Datatype dt,
                  int np, const kf_adam_hyper *hyper, uint32_t key, UpdateGate *g, void *stream)
{
    const int rc = check_update_batch(
        fail, {{params, 16, kOff16}, {grads, 16, kOff16}, {exp_avgs, 16, kOff16},
               {exp_avg_sqs, 16, kOff16}},
        {bases, streams}, counts, nb, np, hyper, g, false,
        [&]() -> int {
            if (dt == KungFu_BFLOAT16) return KF_OK;
            return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE",
                        "bf16 only (f32 and f64 take kf_adam_update_batch; f16 the master path)");
        },
        no_check,
        [&](int b) -> int {
            if (bases[b] % kAdamSrElts != 0) {
                return fail(KF_ERR_ARG, "KF_ERR_ARG", "bases must be multiples of 8 elements");
            }
            if (bases[b] > kMaxElement || counts[b] > kMaxElement - bases[b]) {
                return fail(KF_ERR_ARG, "KF_ERR_ARG", "base + count must be at most 2^33");
            }
            return KF_OK;
        });
    if (rc != KF_OK || nb == 0) return rc;
    return launch_adam_sr(params, grads, exp_avgs, exp_avg_sqs, counts, bases, streams, nb, np,
                          hyper, key, static_cast<hipStream_t>(stream), g ? g->gate : nullptr,
                          g ? g->state : nullptr);
}

}  // namespace

extern "C" {

int kf_adam_sr_update_batch(void *const *params, const void *const *grads, void *const *exp_avgs,
                            void *const *exp_avg_sqs, const size_t *counts, const uint64_t *bases,
                            const uint32_t *streams, int nb, KungFu_Datatype dt, int np,
                            const kf_adam_hyper *hyper, uint32_t key, void *stream)
{
    return adam_sr_entry(fail, params, grads, exp_avgs, exp_avg_sqs, counts, bases, streams, nb, dt,
                         np, hyper, key, nullptr, stream);
}

int kf_adam_sr_update_batch_gated(void *const *params, const void *const *grads,
                                  void *const *exp_avgs, void *const *exp_avg_sqs,
                                  const size_t *counts, const uint64_t *bases,
                                  const uint32_t *streams, int nb, KungFu_Datatype dt, int np,
                                  const kf_adam_hyper *hyper, uint32_t key,
                                  const kf_step_gate *gate, const kf_step_state *state,
                                  void *stream)
{
    UpdateGate g = {gate, state, {}};
    return adam_sr_entry(fail_gated, params, grads, exp_avgs, exp_avg_sqs, counts, bases, streams,
                         nb, dt, np, hyper, key, &g, stream);
}

int kf_adam_sr_narrow(const void *x, const void *r, void *out, size_t n, void *stream)
{
    if (n == 0) return KF_OK;
    if (!x || !r || !out) return fail_narrow(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    if (reinterpret_cast<uintptr_t>(x) % 4 || reinterpret_cast<uintptr_t>(r) % 2 ||
        reinterpret_cast<uintptr_t>(out) % 2) {
        return fail_narrow(KF_ERR_ARG, "KF_ERR_ARG", "pointers must be aligned to their elements");
    }
    const size_t blocks = ((n + 1) / 2 + 255) / 256;
    const unsigned grid = static_cast<unsigned>(blocks < 65536 ? blocks : 65536);
    adam_sr_narrow_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint32_t *>(x), static_cast<const uint16_t *>(r),
        static_cast<uint16_t *>(out), n);
    return launch_status(fail_narrow);
}

}  // extern "C"
