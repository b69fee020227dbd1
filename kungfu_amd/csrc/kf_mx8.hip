// kf_mx8.hip — the MXFP8 gradient wire (include/kungfu_amd.h "MXFP8 gradient
// wire"): what phase 1 of a sharded step carries when the
// exchange's gradient wire is "mx8" (ZeRO++'s quantized gradient all-to-all,
// with CDNA4's OCP microscaling format in place of int8 / int4):
//
//   [pack: every bucket's world pieces -> E4M3 codes + E8M0 scales]
//     -> all-to-all of the packed pieces
//     -> [fold: the world received pieces of this rank's shard, decoded and
//         added in f32 in rank order, /np, one narrowing] -> the shard
//
// A block is 32 consecutive elements: 32 one-byte E4M3 codes and one scale
// byte, the biased exponent of a power of two (E8M0). A piece of q elements
// is q code bytes, then q / 32 scale bytes, then zeros up to the next 16
// bytes: 1.03125 bytes per element against 4 (f32) or 2 (bf16, f16).
//
// The pack kernel. kf_update_batch.hpp's batched launch, one segment per
// (bucket, piece), 256 lanes. A lane owns 8 consecutive elements (two 16-byte
// non-temporal loads of f32, one of 16-bit), so a block is the 4 lanes of a
// DPP quad and a wave's tile is 512 elements = 16 blocks. The block's largest
// magnitude is an unsigned integer maximum over the quad (two quad_perm
// steps; integer, so that a NaN or inf wins, as in kf_adam8.hip): no LDS, no
// barrier. The codes come from v_cvt_scalef32_pk_fp8_f32, which takes the
// scale byte in the exponent field of an f32; they leave as one 8-byte store
// per lane. The 16 scale bytes of a wave's tile are shifted to their place in
// a dword per DPP row (two row_ror steps), read out of the four rows with
// v_readlane and stored by the wave's first lane as one 16-byte store. A
// shard that ends inside a tile runs the same code: its missing quads load
// nothing, take part in the cross-lane steps as all-zero blocks and store no
// codes, and the scale store's surplus bytes are the piece's zero padding
// (q % 32 == 0 keeps a quad inside the shard or outside it as a whole).
//
// The fold kernel. One segment per bucket, 256 lanes, a lane owns 16
// consecutive elements (half a block): per rank one 16-byte load of codes, the
// block's scale byte (one byte load; the two lanes of a block and their
// neighbours share the cache line), and eight v_cvt_scalef32_pk_f32_fp8 into
// 16 f32 values that are added to 16 accumulators. Rank r + 1's codes and
// scale are loaded before rank r's are decoded, so one rank's load is in
// flight behind the arithmetic: shards are small launches, where the k-input
// fold of kf_reduce_kernels.hpp measured more loads in flight ahead of one
// (DESIGN.md §10), and the 20 bytes a lane keeps in flight here are what 16
// elements of a rank cost at all. The /np mode is a template parameter
// (kf_lars.hip). Stores are 4 x 16 bytes (f32) or 2 x 16 bytes (bf16, f16).
//
// The scaled conversions and the definition. Both instructions read the scale
// byte from the exponent field of an f32 operand (byte << 23, whatever the
// value means as a float) and agree with the definition over the whole scale
// range: subnormal f32 inputs, the clamped exponent -127 (byte 0) and
// unpacked values that are f32 subnormals included (DESIGN.md §24 has the
// probe's rows). Only the block that is not finite is handled in plain ALU:
//   * pack: its scale byte is 0xFF by the integer maximum, and its codes are
//     zeros by a select (the instruction would write E4M3's NaN code);
//   * unpack: its elements are the one quiet NaN 0x7fc00000 by a select (the
//     instruction gives a NaN with the sign bit set).
//
// No contraction (the pragma of kf_reduce_kernels.hpp and -ffp-contract=off),
// no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_sgd_elt.hpp"
#include "kf_update_batch.hpp"

namespace kf
{
constexpr int kMx8Block    = 256;  // lanes
constexpr int kMx8Blk      = 32;   // elements per scale byte
constexpr int kMx8PackElts = 8;    // elements per lane, pack: a block is a quad
constexpr int kMx8FoldElts = 16;   // elements per lane, fold: half a block
constexpr int kMx8Seg      = 32;   // segments per launch
static_assert(kMx8Blk == 4 * kMx8PackElts, "a block is one DPP quad");

typedef short mx8_i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int mx8_u32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned kMx8NaN = 0x7fc00000u;  // what a block of scale 0xFF unpacks to

// ---- the format, per block ------------------------------------------------------

// the scale byte of a block whose largest magnitude has the bits `mag`
__device__ __forceinline__ unsigned mx8_scale_byte(unsigned mag)
{
    if (mag >= 0x7f800000u) return 0xffu;
    const unsigned k = (mag + 0x00200000u) >> 23;  // the exponent, + 1 from a fraction of 0.75
    return max(k, 8u) - 8u;                        // e + 127, e = max(k - 135, -127); k <= 255
}

// the maximum of k over the lane's quad, in every lane of the quad
__device__ __forceinline__ unsigned mx8_quad_max(unsigned k)
{
    // quad_perm:[1,0,3,2], then [2,3,0,1]
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0xb1, 0xf, 0xf, false)));
    k = max(k, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(k), 0x4e, 0xf, 0xf, false)));
    return k;
}

// The 16 scale bytes of a wave's tile, quad j's in byte j, in every lane.
// Every lane of the wave must be here; `byte` is uniform over a quad.
__device__ __forceinline__ u32x4 mx8_wave_scales(unsigned byte)
{
    const unsigned lane = threadIdx.x & 63u;
    unsigned t          = byte << (8u * ((lane >> 2) & 3u));  // its place in the row's dword
    // row_ror:4, then row_ror:8: the other three quads of the row
    t |= static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(t), 0x124, 0xf, 0xf, false));
    t |= static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(t), 0x128, 0xf, 0xf, false));
    const int v = static_cast<int>(t);
    return u32x4{static_cast<unsigned>(__builtin_amdgcn_readlane(v, 0)),
                 static_cast<unsigned>(__builtin_amdgcn_readlane(v, 16)),
                 static_cast<unsigned>(__builtin_amdgcn_readlane(v, 32)),
                 static_cast<unsigned>(__builtin_amdgcn_readlane(v, 48))};
}

// four elements -> four codes in a dword, element j in byte j
__device__ __forceinline__ unsigned mx8_cvt4(float a, float b, float c, float d, float scale)
{
    mx8_i16x2 r = {0, 0};
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, a, b, scale, false);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, c, d, scale, true);
    return __builtin_bit_cast(unsigned, r);
}

// ---- pack ---------------------------------------------------------------------
struct Mx8PackSeg {
    const void *src;  // the piece's q elements inside the gradient bucket
    void *dst;        // the piece: q codes, q / 32 scales, zeros to the next 16 bytes
    size_t n;         // q
};
struct Mx8PackArgs {
    Mx8PackSeg seg[kMx8Seg];
    unsigned blk0[kMx8Seg + 1];
    int nseg;
};
static_assert(sizeof(Mx8PackArgs) <= 1024, "kernarg budget");

// the lane's 8 elements, widened (exactly); zeros outside the shard
template <typename T>
__device__ __forceinline__ void mx8_load8(const void *src, size_t u, bool active, float (&x)[8])
{
    u32x4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0};
    if constexpr (std::is_same<T, float>::value) {
        if (active) {
            r0 = ld_u4<1>(src, 2 * u);
            r1 = ld_u4<1>(src, 2 * u + 1);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i]     = __uint_as_float(r0[i]);
            x[4 + i] = __uint_as_float(r1[i]);
        }
    } else {
        if (active) r0 = ld_u4<1>(src, u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i]     = SgdElt<T>::widen(static_cast<uint16_t>(r0[i]));
            x[2 * i + 1] = SgdElt<T>::widen(static_cast<uint16_t>(r0[i] >> 16));
        }
    }
}

template <typename T>
__device__ __forceinline__ void mx8_pack_body(const Mx8PackSeg &h, size_t blk, size_t nblk)
{
    constexpr int B     = kMx8Block;
    const size_t nunit  = h.n / kMx8PackElts;
    const size_t ntiles = (nunit + B - 1) / B;
    char *codes         = static_cast<char *>(h.dst);
    char *scales        = codes + h.n;
    // uniform over the workgroup: every lane takes every cross-lane step
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u    = t * B + threadIdx.x;
        const bool active = u < nunit;  // uniform over a quad: n % 32 == 0
        float x[8];
        mx8_load8<T>(h.src, u, active, x);
        unsigned mag = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) mag = max(mag, __float_as_uint(x[i]) & 0x7fffffffu);
        const unsigned byte = mx8_scale_byte(mx8_quad_max(mag));
        const float scale = __uint_as_float(byte << 23);  // the instruction reads the exponent field
        mx8_u32x2 out     = {mx8_cvt4(x[0], x[1], x[2], x[3], scale),
                             mx8_cvt4(x[4], x[5], x[6], x[7], scale)};
        if (byte == 0xffu) out = mx8_u32x2{0, 0};
        const u32x4 sc = mx8_wave_scales(byte);
        if (active) reinterpret_cast<mx8_u32x2 *>(codes)[u] = out;
        const size_t uw = u & ~static_cast<size_t>(63);  // the wave's first unit
        if ((threadIdx.x & 63u) == 0 && uw < nunit) st_u4<0>(scales, uw / 64, sc);
    }
}

template <typename T> __global__ void __launch_bounds__(kMx8Block) mx8_pack_kernel(Mx8PackArgs a)
{
    size_t blk, nblk;
    const Mx8PackSeg &g = a.seg[batch_segment(a, blk, nblk)];
    mx8_pack_body<T>(g, blk, nblk);
}

// ---- fold ---------------------------------------------------------------------
struct Mx8FoldSeg {
    const void *pk;  // the world received pieces of this rank's shard, `stride` apart
    void *out;       // the shard, in the bucket's dtype
    size_t n;        // q
    size_t stride;   // kf_mx8_piece_bytes(q)
};
struct Mx8FoldArgs {
    Mx8FoldSeg seg[kMx8Seg];
    unsigned blk0[kMx8Seg + 1];
    int nseg;
};
static_assert(sizeof(Mx8FoldArgs) + sizeof(Div) <= 1536, "kernarg budget");

struct Mx8Raw {
    u32x4 codes;
    unsigned byte;
};

__device__ __forceinline__ Mx8Raw mx8_fold_load(const char *piece, size_t n, size_t u)
{
    Mx8Raw r;
    r.codes = ld_u4<1>(piece, u);
    r.byte  = reinterpret_cast<const uint8_t *>(piece + n)[u >> 1];
    return r;
}

__device__ __forceinline__ void mx8_decode16(const Mx8Raw &r, float (&v)[16])
{
    const float scale = __uint_as_float(r.byte << 23);  // the instruction reads the exponent field
    const bool nan    = r.byte == 0xffu;
    const float qnan  = __uint_as_float(kMx8NaN);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(r.codes[w], scale, false);
        const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(r.codes[w], scale, true);
        v[4 * w]       = nan ? qnan : lo.x;
        v[4 * w + 1]   = nan ? qnan : lo.y;
        v[4 * w + 2]   = nan ? qnan : hi.x;
        v[4 * w + 3]   = nan ? qnan : hi.y;
    }
}

// the one narrowing of a finished f32 value: never fused with the operation
// that made it (kf_reduce_kernels.hpp f32_product_to_f16)
template <typename T> __device__ __forceinline__ uint16_t mx8_narrow(float s)
{
    asm("" : "+v"(s));
    return SgdElt<T>::narrow(s);
}

template <typename T, int DIV>
__device__ __forceinline__ void mx8_fold_body(const Mx8FoldSeg &h, int world, const Div &d,
                                              size_t blk, size_t nblk)
{
    constexpr int B     = kMx8Block;
    const size_t nunit  = h.n / kMx8FoldElts;
    const size_t ntiles = (nunit + B - 1) / B;
    const char *pk      = static_cast<const char *>(h.pk);
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u = t * B + threadIdx.x;
        if (u >= nunit) continue;
        float acc[16], v[16];
        Mx8Raw cur = mx8_fold_load(pk, h.n, u);
        for (int r = 0; r < world; ++r) {
            Mx8Raw next = cur;
            if (r + 1 < world) next = mx8_fold_load(pk + (r + 1) * h.stride, h.n, u);
            mx8_decode16(cur, v);
            if (r == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = v[i];
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = __fadd_rn(acc[i], v[i]);
            }
            cur = next;
        }
        if constexpr (DIV != 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = SgdElt<float>::div<DIV == 1>(acc[i], d);
        }
        if constexpr (std::is_same<T, float>::value) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                st_u4<0>(h.out, 4 * u + w,
                         u32x4{__float_as_uint(acc[4 * w]), __float_as_uint(acc[4 * w + 1]),
                               __float_as_uint(acc[4 * w + 2]), __float_as_uint(acc[4 * w + 3])});
            }
        } else {
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                u32x4 raw;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    raw[i] = static_cast<unsigned>(mx8_narrow<T>(acc[8 * w + 2 * i])) |
                             (static_cast<unsigned>(mx8_narrow<T>(acc[8 * w + 2 * i + 1])) << 16);
                }
                st_u4<0>(h.out, 2 * u + w, raw);
            }
        }
    }
}

template <typename T, int DIV>
__global__ void __launch_bounds__(kMx8Block) mx8_fold_kernel(Mx8FoldArgs a, int world, Div np)
{
    size_t blk, nblk;
    const Mx8FoldSeg &g = a.seg[batch_segment(a, blk, nblk)];
    mx8_fold_body<T, DIV>(g, world, np, blk, nblk);
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail_pack{"kf_mx8_pack_batch"};
constexpr UpdateFail fail_fold{"kf_mx8_fold_batch"};

size_t piece_bytes(size_t q) { return (q + q / kMx8Blk + 15) / 16 * 16; }

// What both entries check, in the header's order, before any HIP call;
// q(b): bucket b's shard length.
template <typename Q>
int mx8_check(const UpdateFail &fail, const void *const *a, const void *const *b,
              const size_t *counts, int nb, int world, KungFu_Datatype dt, int np, Q &&q)
{
    if (nb < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "nb < 0");
    if (nb == 0) return KF_OK;
    if (!a || !b || !counts) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    if (dt != KungFu_FLOAT && dt != KungFu_BFLOAT16 && dt != KungFu_FLOAT16) {
        return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "f32, bf16 and f16 only");
    }
    if (world < 1 || world > KF_MAX_INPUTS) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "world must be in [1, 16]");
    }
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    for (int i = 0; i < nb; ++i) {
        if (q(i) == 0) continue;
        if (!a[i] || !b[i]) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty bucket");
        if (q(i) % kMx8Blk) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "shard lengths must be multiples of 32 (a block)");
        }
        if (off16(a[i]) || off16(b[i])) return fail(KF_ERR_ARG, "KF_ERR_ARG", kOff16);
    }
    return KF_OK;
}

template <typename T>
int launch_pack(const void *const *grads, void *const *packed, const size_t *counts, int nb,
                int world, hipStream_t s)
{
    // one segment per (bucket, piece)
    const size_t W = static_cast<size_t>(world);
    std::vector<size_t> qs(static_cast<size_t>(nb) * W);
    for (size_t i = 0; i < qs.size(); ++i) qs[i] = counts[i / W] / W;
    return plan_update_batch<Mx8PackArgs>(
        qs.data(), static_cast<int>(qs.size()), kMx8PackElts, kMx8Block,
        [&](Mx8PackSeg &g, int i) {
            const size_t b = i / W, j = i % W, q = qs[i];
            g.src = static_cast<const char *>(grads[b]) + j * q * sizeof(typename SgdElt<T>::S);
            g.dst = static_cast<char *>(packed[b]) + j * piece_bytes(q);
            g.n   = q;
        },
        [&](unsigned gx, unsigned gy, const Mx8PackArgs &a) {
            mx8_pack_kernel<T><<<dim3(gx, gy), kMx8Block, 0, s>>>(a);
            return launch_status(fail_pack);
        });
}

template <typename T, int DIV>
int launch_fold(const void *const *packed, void *const *outs, const size_t *q, int nb, int world,
                const Div &dv, hipStream_t s)
{
    return plan_update_batch<Mx8FoldArgs>(
        q, nb, kMx8FoldElts, kMx8Block,
        [&](Mx8FoldSeg &g, int b) {
            g.pk     = packed[b];
            g.out    = outs[b];
            g.n      = q[b];
            g.stride = piece_bytes(q[b]);
        },
        [&](unsigned gx, unsigned gy, const Mx8FoldArgs &a) {
            mx8_fold_kernel<T, DIV><<<dim3(gx, gy), kMx8Block, 0, s>>>(a, world, dv);
            return launch_status(fail_fold);
        });
}

template <typename T>
int launch_fold_div(const void *const *packed, void *const *outs, const size_t *q, int nb,
                    int world, int np, hipStream_t s)
{
    const Div dv = update_div(np);
    switch (update_div_code(np, dv)) {
    case 0: return launch_fold<T, 0>(packed, outs, q, nb, world, dv, s);
    case 1: return launch_fold<T, 1>(packed, outs, q, nb, world, dv, s);
    default: return launch_fold<T, 2>(packed, outs, q, nb, world, dv, s);
    }
}

}  // namespace

extern "C" {

size_t kf_mx8_piece_bytes(size_t q) { return piece_bytes(q); }

int kf_mx8_pack_batch(const void *const *grads, void *const *packed, const size_t *counts, int nb,
                      int world, KungFu_Datatype dt, void *stream)
{
    const int rc = mx8_check(fail_pack, grads, packed, counts, nb, world, dt, 0,
                             [&](int b) { return counts[b] / static_cast<size_t>(world); });
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) return launch_pack<float>(grads, packed, counts, nb, world, s);
    if (dt == KungFu_BFLOAT16) return launch_pack<bf16_t>(grads, packed, counts, nb, world, s);
    return launch_pack<f16_t>(grads, packed, counts, nb, world, s);
}

int kf_mx8_fold_batch(const void *const *packed, void *const *out_shards, const size_t *q, int nb,
                      int world, KungFu_Datatype dt, int np, void *stream)
{
    const int rc = mx8_check(fail_fold, packed, out_shards, q, nb, world, dt, np,
                             [&](int b) { return q[b]; });
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) return launch_fold_div<float>(packed, out_shards, q, nb, world, np, s);
    if (dt == KungFu_BFLOAT16) {
        return launch_fold_div<bf16_t>(packed, out_shards, q, nb, world, np, s);
    }
    return launch_fold_div<f16_t>(packed, out_shards, q, nb, world, np, s);
}

}  // extern "C"
