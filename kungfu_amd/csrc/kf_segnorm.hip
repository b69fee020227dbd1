// kf_segnorm.hip — segmented squared-norm reduction and the noise-scale update
// (include/kungfu_amd.h "gradient monitors"): what the two monitoring
// optimizers (grad_noise_scale.py, grad_variance.py) need beyond the sync
// reduce — many tensors, each reduced to one fp64 scalar, in one read-only
// pass over the gradient buckets.
//
// One plan (kf_segnorm_create) holds a segment table in HBM: per segment its
// pointers, its count and its first block. A run is two or three launches:
//   1. segnorm_kernel: block b finds its segment by binary search of the
//      table (214 tensors of ResNet-50 are one launch, not 14 kernarg-limited
//      ones), streams its tiles with 16-B non-temporal loads, accumulates in
//      fp64 from the first add (convert, then fma(x, x, acc) per lane) and
//      writes ONE fp64 partial with a plain store;
//   2. segnorm_fold_kernel: one block per segment adds that segment's
//      partials in block order with a fixed tree -> out[s];
//   3. segnorm_total_kernel: out[nseg] = out[0] + out[1] + ... left to right
//      (or of their square roots). With one segment, launch 2 writes it.
// No float atomics and no in-launch ticket: the launch boundary orders the
// partials, every partial read was written by the same run, so the same plan
// and input bytes give the same output bits whatever the workspace held.
//
// Error bound: squares of <= 24-bit significands are exact in fp64 and every
// add is one rounding of a non-negative sum, so |out[s] - exact| <=
// (n - 1) * 2^-53 * exact for f32 / f16 / bf16; an fp64 input's fma rounds
// its square and the add once, still within (n + 2) * 2^-53.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "kf_reduce_kernels.hpp"
#include "kungfu_amd.h"

namespace kf
{
void set_last_error(const std::string &msg);  // kf_capi.hip: kf_last_error's text

// One row of the device table; row nseg is a sentinel whose blk0 is the grid.
struct SegDesc {
    const void *a;
    const void *b;
    size_t n;
    unsigned blk0;  // the segment's first block; it owns [blk0, next row's blk0)
    unsigned pad_;
};
static_assert(sizeof(SegDesc) == 32, "table row");

enum { NORM_SQ = 0, NORM_VAR = 1 };

// The term whose square is summed, widened (exactly) to fp64.
//   sq:  a
//   var: fl_T(a - fl_T(b * b)), each operation rounded to T, no contraction
//        (grad_variance.py:51-54 in the tensor's own dtype); f16 / bf16
//        compute in fp32 and round to T after the multiply and the subtract.
template <typename T> struct NormElt;
template <> struct NormElt<float> {
    using S = float;
    __device__ static double sq(S a) { return static_cast<double>(a); }
    __device__ static double var(S a, S b)
    {
        return static_cast<double>(__fsub_rn(a, __fmul_rn(b, b)));
    }
};
template <> struct NormElt<double> {
    using S = double;
    __device__ static double sq(S a) { return a; }
    __device__ static double var(S a, S b) { return __dsub_rn(a, __dmul_rn(b, b)); }
};
template <> struct NormElt<f16_t> {
    using S = uint16_t;
    __device__ static double sq(S a) { return static_cast<double>(f16_to_f32(a)); }
    __device__ static double var(S a, S b)
    {
        const float fb = f16_to_f32(b);
        // compiled to the native v_mul_f16 / v_sub_f16 (same value); a square
        // is never -0, so the x * y + 0 form could not hurt it either
        const float p  = f16_to_f32(f32_to_f16(__fmul_rn(fb, fb)));
        return static_cast<double>(f16_to_f32(f32_to_f16(__fsub_rn(f16_to_f32(a), p))));
    }
};
template <> struct NormElt<bf16_t> {
    using S = uint16_t;
    __device__ static double sq(S a) { return static_cast<double>(bf16_to_f32(a)); }
    __device__ static double var(S a, S b)
    {
        const float fb = bf16_to_f32(b);
        const float p  = bf16_to_f32(f32_to_bf16(__fmul_rn(fb, fb)));
        return static_cast<double>(bf16_to_f32(f32_to_bf16(__fsub_rn(bf16_to_f32(a), p))));
    }
};

// The segment pointers come out of the table in memory, where the compiler
// cannot see that they are global: left generic, every load is a flat_load.
// They are HBM (or host-mapped) addresses by contract, so they are cast to the
// global address space, and ld_g4 is ld_u4<1> on such a pointer:
// global_load_dwordx4 ... nt.
#define KF_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ u32x4 ld_g4(const KF_GLOBAL char *base, size_t vi)
{
    return __builtin_nontemporal_load(reinterpret_cast<const KF_GLOBAL u32x4 *>(base) + vi);
}

constexpr int kNormBlock = 256;
constexpr int kNormAcc   = 4;  // independent fp64 accumulators per lane
// 16-B vectors per lane per tile: eight loads in flight per lane either way
// (reduce_body's k = 2 tile has the same eight)
constexpr int kNormUnrollSq  = 8;
constexpr int kNormUnrollVar = 4;

// The block's lanes -> one value, in a fixed order: shuffles inside a wave,
// the four waves through LDS, added left to right by thread 0 (which alone
// holds the result).
template <int BLOCK> __device__ __forceinline__ double block_sum(double v, double *lds)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = lds[0];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) r = __dadd_rn(r, lds[w]);
    }
    return r;
}

template <typename T, int MODE>
__device__ __forceinline__ void norm_vec(const u32x4 &ra, const u32x4 &rb, double (&acc)[kNormAcc])
{
    using S         = typename NormElt<T>::S;
    constexpr int E = 16 / sizeof(S);
    Vec<S> a, b;
    __builtin_memcpy(&a, &ra, 16);
    if constexpr (MODE == NORM_VAR) __builtin_memcpy(&b, &rb, 16);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        double x;
        if constexpr (MODE == NORM_VAR) x = NormElt<T>::var(a.e[e], b.e[e]);
        else x = NormElt<T>::sq(a.e[e]);
        acc[e % kNormAcc] = __fma_rn(x, x, acc[e % kNormAcc]);
    }
}

// Block `blk` of the `nblk` of one segment. Elements [0, head) and
// [head + nvec * E, n) go one per lane of block 0 (fewer than 2 * E of them),
// the rest as 16-B vectors from a's first 16-B boundary; b (VAR) is read at
// the same element offsets, with the same 16-B load at an element-aligned
// address when its residue differs from a's (kf_capi.hip make_plan: gfx950
// queues run in unaligned-access mode).
template <typename T, int MODE, int BLOCK, int UNROLL>
__device__ __forceinline__ double segnorm_body(const SegDesc &d, size_t blk, size_t nblk,
                                               double *lds)
{
    using S         = typename NormElt<T>::S;
    constexpr int E = 16 / sizeof(S);
    const KF_GLOBAL S *pa = (const KF_GLOBAL S *)d.a;
    const KF_GLOBAL S *pb = (const KF_GLOBAL S *)d.b;
    const size_t n  = d.n;
    const size_t r  = reinterpret_cast<uintptr_t>(pa) & 15u;
    size_t head     = r == 0 ? 0 : (16 - r) / sizeof(S);
    if (head > n) head = n;
    const size_t nvec  = (n - head) / E;
    const size_t vend  = head + nvec * E;
    const size_t nedge = head + (n - vend);

    double acc[kNormAcc];
#pragma unroll
    for (int i = 0; i < kNormAcc; ++i) acc[i] = 0.0;

    if (blk == 0 && threadIdx.x < nedge) {
        const size_t t = threadIdx.x;
        const size_t i = t < head ? t : vend + (t - head);
        double x;
        if constexpr (MODE == NORM_VAR) x = NormElt<T>::var(pa[i], pb[i]);
        else x = NormElt<T>::sq(pa[i]);
        acc[0] = __fma_rn(x, x, acc[0]);
    }

    const KF_GLOBAL char *va = reinterpret_cast<const KF_GLOBAL char *>(pa + head);
    const KF_GLOBAL char *vb = reinterpret_cast<const KF_GLOBAL char *>(pb + head);  // VAR only
    const size_t tile   = static_cast<size_t>(BLOCK) * UNROLL;
    const size_t ntiles = (nvec + tile - 1) / tile;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        if (v0 + (UNROLL - 1) * BLOCK < nvec) {
            // full tile: every load issued before the first use
            u32x4 ra[UNROLL], rb[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) ra[u] = ld_g4(va, v0 + u * BLOCK);
            if constexpr (MODE == NORM_VAR) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) rb[u] = ld_g4(vb, v0 + u * BLOCK);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) norm_vec<T, MODE>(ra[u], rb[u], acc);
        } else {
            // ragged last tile
            for (int u = 0; u < UNROLL; ++u) {
                const size_t vi = v0 + u * BLOCK;
                if (vi >= nvec) break;
                u32x4 ra = ld_g4(va, vi), rb = ra;
                if constexpr (MODE == NORM_VAR) rb = ld_g4(vb, vi);
                norm_vec<T, MODE>(ra, rb, acc);
            }
        }
    }
    const double v = __dadd_rn(__dadd_rn(acc[0], acc[1]), __dadd_rn(acc[2], acc[3]));
    return block_sum<BLOCK>(v, lds);
}

// Launch 1. Block b works for the last segment s whose blk0 <= b: segments
// without blocks (count 0) share their blk0 with the next one that has some,
// and the search lands on that one.
template <typename T, int MODE>
__global__ void __launch_bounds__(kNormBlock)
    segnorm_kernel(const SegDesc *__restrict__ seg, int nseg, double *__restrict__ partials)
{
    __shared__ double lds[kNormBlock / 64];
    const unsigned b = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b >= seg[mid].blk0) lo = mid;
        else hi = mid - 1;
    }
    const SegDesc d     = seg[lo];
    const unsigned next = seg[lo + 1].blk0;
    constexpr int U     = MODE == NORM_VAR ? kNormUnrollVar : kNormUnrollSq;
    const double v = segnorm_body<T, MODE, kNormBlock, U>(d, b - d.blk0, next - d.blk0, lds);
    if (threadIdx.x == 0) partials[b] = v;
}

// Launch 2: block s adds segment s's partials. Lane i takes partials i,
// i + 256, ... in order (eight loads at a time), then block_sum's tree.
// `single` (nseg == 1): the total is out[0] itself, written here.
__global__ void __launch_bounds__(kNormBlock)
    segnorm_fold_kernel(const SegDesc *__restrict__ seg, const double *__restrict__ partials,
                        double *__restrict__ out, int single, int total_sqrt)
{
    __shared__ double lds[kNormBlock / 64];
    constexpr int G   = 8;
    const unsigned s  = blockIdx.x;
    const size_t b0   = seg[s].blk0, b1 = seg[s + 1].blk0;
    double v          = 0.0;
    size_t i          = b0 + threadIdx.x;
    for (; i + (G - 1) * kNormBlock < b1; i += G * kNormBlock) {
        double x[G];
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] = partials[i + g * kNormBlock];
#pragma unroll
        for (int g = 0; g < G; ++g) v = __dadd_rn(v, x[g]);
    }
    for (; i < b1; i += kNormBlock) v = __dadd_rn(v, partials[i]);
    const double r = block_sum<kNormBlock>(v, lds);
    if (threadIdx.x == 0) {
        out[s] = r;
        if (single) out[1] = total_sqrt ? __dsqrt_rn(r) : r;
    }
}

// Launch 3: out[nseg] = ((out[0] + out[1]) + out[2]) + ..., or the same sum
// of sqrt(out[s]). One block: 256 values staged in LDS at a time, added in
// index order by thread 0.
__global__ void __launch_bounds__(kNormBlock)
    segnorm_total_kernel(double *__restrict__ out, int nseg, int total_sqrt)
{
    __shared__ double buf[kNormBlock];
    double tot = 0.0;
    for (int base = 0; base < nseg; base += kNormBlock) {
        const int i = base + static_cast<int>(threadIdx.x);
        double x    = 0.0;
        if (i < nseg) x = total_sqrt ? __dsqrt_rn(out[i]) : out[i];
        buf[threadIdx.x] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = nseg - base < kNormBlock ? nseg - base : kNormBlock;
            for (int j = 0; j < m; ++j) tot = __dadd_rn(tot, buf[j]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[nseg] = tot;
}

// monitor.py:10-17, ema.hpp:19-27, collective.cpp:298-300 in fp32, one lane,
// no contraction. state = {g_ema, s_ema, noise_scale, has_value}.
__global__ void noise_scale_kernel(const double *__restrict__ sq_small,
                                   const double *__restrict__ sq_big, float bs, float bb,
                                   float alpha, float *__restrict__ state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float Gs = static_cast<float>(*sq_small);
    const float Gb = static_cast<float>(*sq_big);
    const float G  = __fmul_rn(__fdiv_rn(1.0f, __fsub_rn(bb, bs)),
                               __fsub_rn(__fmul_rn(bb, Gb), __fmul_rn(bs, Gs)));
    const float S  = __fmul_rn(
        __fdiv_rn(1.0f, __fsub_rn(__fdiv_rn(1.0f, bs), __fdiv_rn(1.0f, bb))), __fsub_rn(Gs, Gb));
    float g = G, s = S;
    if (state[3] != 0.0f) {
        const float c = __fsub_rn(1.0f, alpha);
        g = __fadd_rn(__fmul_rn(alpha, state[0]), __fmul_rn(c, G));
        s = __fadd_rn(__fmul_rn(alpha, state[1]), __fmul_rn(c, S));
    }
    state[0] = g;
    state[1] = s;
    state[2] = __fdiv_rn(s, g);
    state[3] = 1.0f;
}

}  // namespace kf

struct kf_segnorm {
    kf::SegDesc *seg  = nullptr;  // device, nseg + 1 rows
    double *partials  = nullptr;  // device, one per block of launch 1
    int nseg          = 0;
    unsigned blocks   = 0;
    bool has_b        = false;
    KungFu_Datatype dt = KungFu_FLOAT;
};

namespace
{
using namespace kf;

// Bytes of `a` per block of launch 1 (one SQ tile), and the most blocks one
// segment gets; past that its blocks stride over the tiles. The cap keeps the
// fold of a large segment to one round of loads per lane
// (KUNGFU_AMD_SEGNORM_MAX_BLOCKS overrides it, for tools/bench_segnorm.py).
constexpr size_t kBytesPerBlock = static_cast<size_t>(kNormBlock) * kNormUnrollSq * 16;
constexpr unsigned kSegMaxBlocks = 2048;

unsigned seg_max_blocks()
{
    const char *e = std::getenv("KUNGFU_AMD_SEGNORM_MAX_BLOCKS");
    const long v  = e ? std::atol(e) : 0;
    return v >= 1 && v <= (1 << 20) ? static_cast<unsigned>(v) : kSegMaxBlocks;
}

int fail(int rc, const char *name, const std::string &what)
{
    set_last_error(std::string(name) + ": " + what);
    return rc;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(KF_ERR_HIP, "KF_ERR_HIP", std::string(what) + ": " + hipGetErrorString(e));
}

int elt_size(KungFu_Datatype dt)
{
    switch (dt) {
    case KungFu_FLOAT16: case KungFu_BFLOAT16: return 2;
    case KungFu_FLOAT: return 4;
    case KungFu_DOUBLE: return 8;
    default: return 0;
    }
}

template <typename T> void launch_norm(const kf_segnorm *p, int var, hipStream_t s)
{
    if (var) segnorm_kernel<T, NORM_VAR><<<p->blocks, kNormBlock, 0, s>>>(p->seg, p->nseg, p->partials);
    else segnorm_kernel<T, NORM_SQ><<<p->blocks, kNormBlock, 0, s>>>(p->seg, p->nseg, p->partials);
}

}  // namespace

extern "C" {

kf_segnorm_t *kf_segnorm_create(const void *const *a, const void *const *b, const size_t *counts,
                                int nseg, KungFu_Datatype dt)
{
    if (nseg <= 0) {
        fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_create: nseg must be at least 1");
        return nullptr;
    }
    if (!a || !counts) {
        fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_create: null segment table");
        return nullptr;
    }
    const int sz = elt_size(dt);
    if (sz == 0) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "kf_segnorm_create: f32, f16, bf16 and f64 only");
        return nullptr;
    }
    const unsigned cap = seg_max_blocks();
    std::vector<SegDesc> rows(static_cast<size_t>(nseg) + 1);
    size_t blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        const size_t n = counts[s];
        if (n && (!a[s] || (b && !b[s]))) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_create: null pointer in a non-empty segment");
            return nullptr;
        }
        if ((n && reinterpret_cast<uintptr_t>(a[s]) % sz) ||
            (n && b && reinterpret_cast<uintptr_t>(b[s]) % sz)) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_create: pointer not aligned to the element");
            return nullptr;
        }
        rows[s].a    = n ? a[s] : nullptr;
        rows[s].b    = n && b ? b[s] : nullptr;
        rows[s].n    = n;
        rows[s].blk0 = static_cast<unsigned>(blocks);
        rows[s].pad_ = 0;
        // blocks in proportion to the bytes, at least one when non-empty
        size_t nb = (n * sz + kBytesPerBlock - 1) / kBytesPerBlock;
        if (nb > cap) nb = cap;
        blocks += nb;
        if (blocks > 0x7fffffffu) {
            fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_create: more than 2^31 - 1 blocks");
            return nullptr;
        }
    }
    rows[nseg]      = SegDesc{nullptr, nullptr, 0, static_cast<unsigned>(blocks), 0};
    kf_segnorm *p   = new kf_segnorm;
    p->nseg         = nseg;
    p->blocks       = static_cast<unsigned>(blocks);
    p->has_b        = b != nullptr;
    p->dt           = dt;
    const size_t tb = rows.size() * sizeof(SegDesc);
    hipError_t e    = hipMalloc(reinterpret_cast<void **>(&p->seg), tb);
    if (e == hipSuccess) {
        e = hipMalloc(reinterpret_cast<void **>(&p->partials),
                      (blocks ? blocks : 1) * sizeof(double));
    }
    if (e == hipSuccess) e = hipMemcpy(p->seg, rows.data(), tb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hip_fail(e, "kf_segnorm_create");
        kf_segnorm_destroy(p);
        return nullptr;
    }
    return p;
}

int kf_segnorm_run(kf_segnorm_t *p, int mode, double *out, void *stream)
{
    if (!p || !out) return fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_run: null plan or out");
    const int what = mode & ~KF_NORM_TOTAL_SQRT;
    if (what != KF_NORM_SQ && what != KF_NORM_VAR) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_run: unknown mode");
    }
    if (what == KF_NORM_VAR && !p->has_b) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_segnorm_run: KF_NORM_VAR needs a plan with b");
    }
    hipStream_t s  = static_cast<hipStream_t>(stream);
    const int var  = what == KF_NORM_VAR;
    const int root = (mode & KF_NORM_TOTAL_SQRT) != 0;
    if (p->blocks) {
        switch (p->dt) {
        case KungFu_FLOAT: launch_norm<float>(p, var, s); break;
        case KungFu_DOUBLE: launch_norm<double>(p, var, s); break;
        case KungFu_FLOAT16: launch_norm<f16_t>(p, var, s); break;
        default: launch_norm<bf16_t>(p, var, s); break;
        }
    }
    const int single = p->nseg == 1;
    segnorm_fold_kernel<<<static_cast<unsigned>(p->nseg), kNormBlock, 0, s>>>(
        p->seg, p->partials, out, single, root);
    if (!single) segnorm_total_kernel<<<1, kNormBlock, 0, s>>>(out, p->nseg, root);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "kf_segnorm_run launch");
    return KF_OK;
}

void kf_segnorm_destroy(kf_segnorm_t *p)
{
    if (!p) return;
    if (p->seg) (void)hipFree(p->seg);
    if (p->partials) (void)hipFree(p->partials);
    delete p;
}

int kf_noise_scale_update(const double *sq_small, const double *sq_big, float batch_small,
                          float batch_big, float alpha, float *state, void *stream)
{
    if (!sq_small || !sq_big || !state) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_noise_scale_update: null pointer");
    }
    if (!(alpha > 0.0f)) {  // collective.cpp:283
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "kf_noise_scale_update: alpha must be greater than zero");
    }
    noise_scale_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        sq_small, sq_big, batch_small, batch_big, alpha, state);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "kf_noise_scale_update launch");
    return KF_OK;
}

}  // extern "C"
